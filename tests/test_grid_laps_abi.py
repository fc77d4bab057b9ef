"""CPU suite for the capped grids (testing notes: laps).  The query engines and the token build launch at most
cu_count() * c workgroups; a wave, or a workgroup, then loops over the work items it was not given first -- one further pass
is a LAP.  tests/test_grid_laps.py sizes its batches and texts from the numbers pinned here, so that a changed cap fails in
this file before the GPU tests silently stop lapping.  Also here, as pure functions: the lap batch (which query a wave meets
on which lap), the gather that assembles a batch's flat arrays from the answers of its distinct queries, and the back-off's
bisection as a probe-counting model."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import test_ngram_abi as ngram_abi
import test_tokens_abi as tokens_abi

WAVE = 64
KINDS = 8                     # kinds of query of the byte batch (the token batch has two more)
TAIL = 37                     # queries of the fourth lap
LAPS = 3                      # full laps of a lap batch


# ---------------------------------------------------------------- the pinned numbers ----

def _source(*path):
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", *path)) as f:
        return f.read()


def kernel_constants(header):
    """every `constexpr int NAME = expression;` of kernels/<header>, evaluated in order -> {name: value}.  The names of the
    headers it builds on (WAVE, the n-gram constants) are known to the expressions."""
    known = {"WAVE": WAVE}
    for dep in {"tokens.hpp": ("ngram.hpp",)}.get(header, ()):
        known.update(kernel_constants(dep))
    for name, expr in re.findall(r"^constexpr int (\w+) = ([^;]+);", _source("kernels", header), re.M):
        known[name] = int(eval(expr, {"__builtins__": {}}, dict(known)))      # noqa: S307 (an integer expression of the project's own source)
    return known


def grid_multiplier(header, function):
    """the c of `cu_count() * c` inside `function` of host/<header>"""
    text = _source("host", header)
    m = re.search(r"\b" + function + r"\([^)]*\)\s*\{(.*?)\n\}", text, re.S)
    assert m, function
    caps = re.findall(r"cu_count\(\) \* (\d+)", m.group(1))
    assert len(caps) == 1, (function, caps)
    return int(caps[0])


NG_THREADS = 256              # kernels/ngram.hpp
DOC_THREADS = 256             # kernels/docs.hpp
DOC_SCAN_TILE = 2048
TK_THREADS = 256              # kernels/tokens.hpp
TK_TILE = 2048
TK_SPAN = 4
TK_IMAGE_ITEMS = 8
TK_IMAGE3_ITEMS = 16          # tokens per work-item of the 3-byte image pass (32-bit tokens)
NGRAM_GRID = 16               # workgroups per CU: ngram_grid
DOCS_UNIT_GRID = 16           # docs_unit_grid
DOC_TF_GRID = 16              # the k_doc_tf launch of doc_tf_query
TOK_STREAM_GRID = 8           # tok_stream_grid


def ngram_waves(cu):
    """W of the query engines: one wave per query"""
    return cu * NGRAM_GRID * (NG_THREADS // WAVE)


def docs_waves(cu):
    """waves of k_doc_count / k_doc_emit: one wave per unit"""
    return cu * DOCS_UNIT_GRID * (DOC_THREADS // WAVE)


def doc_tf_lanes(cu):
    """work-items of k_doc_tf: one per listed entry"""
    return cu * DOC_TF_GRID * DOC_THREADS


def tok_image_lap(cu):
    """tokens one lap of k_tok_be_image takes"""
    return cu * TOK_STREAM_GRID * TK_THREADS * TK_IMAGE_ITEMS


def tok_image3_lap(cu):
    """tokens one lap of k_tok_be_image3 takes"""
    return cu * TOK_STREAM_GRID * TK_THREADS * TK_IMAGE3_ITEMS


def tok_compact_lap(cu):
    """entries of the byte-level array one lap of the compaction kernels takes, whatever the stride: a 16-bit text of n tokens has
    2 n + 1 entries, a 32-bit one 3 n + 1"""
    return cu * TOK_STREAM_GRID * TK_SPAN * TK_TILE


def tok_range_lap(cu):
    """slots one lap of k_tok_sa_range takes"""
    return cu * TOK_STREAM_GRID * TK_THREADS


def tok_id_range_lap(cu):
    """tokens one lap of k_tok_id_range takes: the number of tok_range_lap, from a launch site of its own"""
    return cu * TOK_STREAM_GRID * TK_THREADS


def tok_build_size(cu):
    """tokens of the build that is just past one compaction lap (2 n + 1 entries, a partial last span)"""
    return tok_compact_lap(cu) // 2 + 3 * TK_TILE + 5


def tok32_build_size(cu):
    """tokens of the 32-bit build that is just past one lap of the image pass with a partial last group of 16 tokens; its 3 n + 1
    entries lie between one and two compaction laps with a partial last span and a partial last tile"""
    return tok_image3_lap(cu) + 1369


def test_the_caps_and_the_tiles_are_the_ones_the_gpu_suite_sizes_by():
    ng, docs, tok = kernel_constants("ngram.hpp"), kernel_constants("docs.hpp"), kernel_constants("tokens.hpp")
    assert (ng["NG_THREADS"], ng["NG_WAVES"]) == (NG_THREADS, NG_THREADS // WAVE)
    assert (docs["DOC_THREADS"], docs["DOC_SCAN_TILE"]) == (DOC_THREADS, DOC_SCAN_TILE)
    assert (tok["TK_THREADS"], tok["TK_TILE"], tok["TK_SPAN"], tok["TK_IMAGE_ITEMS"]) == (TK_THREADS, TK_TILE, TK_SPAN, TK_IMAGE_ITEMS)
    assert tok["TK_IMAGE3_ITEMS"] == TK_IMAGE3_ITEMS
    assert (TK_TILE, TK_SPAN) == (tokens_abi.TILE, tokens_abi.SPAN)
    assert grid_multiplier("ngram.hpp", "ngram_grid") == NGRAM_GRID
    assert grid_multiplier("docs.hpp", "docs_unit_grid") == DOCS_UNIT_GRID
    assert grid_multiplier("doc_tf.hpp", "doc_tf_query") == DOC_TF_GRID
    assert grid_multiplier("tokens.hpp", "tok_stream_grid") == TOK_STREAM_GRID
    # the grids the engines are launched with are these functions and no others
    for header, kernel, grid in (("ngram.hpp", "kernel", "ngram_grid(count)"), ("ngram.hpp", "k_infgram_suffix<uint8_t>", "ngram_grid(count)"),
                                 ("tokens.hpp", "k_tok_be_image", "tok_stream_grid(ceil_div(n, TK_IMAGE_ITEMS), TK_THREADS)"),
                                 ("tokens.hpp", "k_tok_sa_range", "tok_stream_grid((int64_t)n + 1, TK_THREADS)"),
                                 ("tokens.hpp", "k_tok_be_image3", "tok_stream_grid(ceil_div(n, TK_IMAGE3_ITEMS), TK_THREADS)"),
                                 ("tokens.hpp", "k_tok_id_range", "tok_stream_grid((int64_t)n, TK_THREADS)"),
                                 ("docs.hpp", "k_doc_count<true>", "docs_unit_grid((int64_t)units)"),
                                 ("docs.hpp", "k_doc_count<false>", "docs_unit_grid((int64_t)b.units)"),
                                 ("docs.hpp", "k_doc_emit", "docs_unit_grid((int64_t)units)")):
        assert re.search(r"hipLaunchKernelGGL\(\(?" + re.escape(kernel) + r"\)?, dim3\(" + re.escape(grid) + r"\)", _source("host", header)), kernel
    host_tok = _source("host", "tokens.hpp")
    assert "const unsigned grid = tok_stream_grid(ceil_div(L.tiles, TK_SPAN), 1);" in host_tok and "const unsigned grid = ngram_grid(count);" in host_tok
    for kernel in ("k_tok_compact_count", "k_tok_compact_scatter", "k_tok_search", "(k_infgram_suffix<uint16_t>)", "(k_infgram_suffix<uint32_t>)"):
        assert "hipLaunchKernelGGL(" + kernel + ", dim3(grid)" in host_tok, kernel
    # each of the 32-bit forms' own kernels is launched from one place: no second site with another grid
    for kernel in ("k_tok_be_image3", "k_tok_id_range", "(k_infgram_suffix<uint32_t>)"):
        assert host_tok.count("hipLaunchKernelGGL(" + kernel + ",") == 1, kernel


def test_the_sizes_on_256_compute_units():
    """the numbers of the issue that asked for these tests, for the MI355X's 256 CUs"""
    assert ngram_waves(256) == docs_waves(256) == 16384 and doc_tf_lanes(256) == 1 << 20
    assert tok_image_lap(256) == 4194304 and tok_compact_lap(256) == 16777216 and tok_range_lap(256) == 524288
    n = tok_build_size(256)
    assert n == 8394757
    length = 2 * n + 1
    assert tok_compact_lap(256) < length < 2 * tok_compact_lap(256)                   # the second lap of the compaction, ...
    tiles = -(-length // TK_TILE)
    assert tiles % TK_SPAN != 0 and length % TK_TILE != 0                               # ... a partial last span and a partial last tile
    assert 2 * tok_image_lap(256) < n <= 3 * tok_image_lap(256)                       # the image pass in its third lap
    assert -(-(tiles + 1) // DOC_SCAN_TILE) == 5                                        # the count scan has five tiles
    assert 2 * n > 4 << 20                                                              # the byte builder is past gram_min_n
    for cu in (1, 8, 104, 256, 304):                                                    # whatever the CU count: the same shape
        n = tok_build_size(cu)
        assert tok_compact_lap(cu) < 2 * n + 1 < 2 * tok_compact_lap(cu) and (-(-(2 * n + 1) // TK_TILE)) % TK_SPAN != 0
        assert n > 2 * tok_image_lap(cu) and tok_range_lap(cu) + 5 < n


def test_the_sizes_of_the_32_bit_build_on_256_compute_units():
    """the same for the build of tests/test_grid_laps32.py: 3 n + 1 entries, 16 tokens a work-item of the image pass"""
    assert tok_image3_lap(256) == 8388608 and tok_id_range_lap(256) == tok_range_lap(256) == 524288
    n = tok32_build_size(256)
    length = 3 * n + 1
    assert (n, length) == (8389977, 25169932)
    assert tok_compact_lap(256) < length < 2 * tok_compact_lap(256)                   # the second lap of the compaction, ...
    tiles = -(-length // TK_TILE)
    assert tiles % TK_SPAN == 3 and length % TK_TILE == 12                              # ... a partial last span and a partial last tile
    assert n % TK_IMAGE3_ITEMS == 9                                                     # a partial last group of the image pass, ...
    assert tok_image3_lap(256) < n < tok_image3_lap(256) + TK_THREADS * TK_IMAGE3_ITEMS # ... which is just past its first lap
    assert -(-(tiles + 1) // DOC_SCAN_TILE) == 7                                        # the count scan has seven tiles
    assert 3 * n > 4 << 20                                                              # the byte builder is past gram_min_n
    assert 1369 % TK_IMAGE3_ITEMS == 9
    for cu in (1, 8, 104, 256, 304):                                                    # whatever the CU count: the same shape
        assert (cu * 98304) % (TK_SPAN * TK_TILE) == 0 and 3 * tok_image3_lap(cu) == cu * 98304
        n = tok32_build_size(cu)
        length = 3 * n + 1
        assert tok_compact_lap(cu) < length < 2 * tok_compact_lap(cu)
        assert (-(-length // TK_TILE)) % TK_SPAN == 3 and length % TK_TILE == 12 and n % TK_IMAGE3_ITEMS == 9
        assert tok_image3_lap(cu) + 5 < n - 1 and (n - 1) // TK_IMAGE3_ITEMS == n // TK_IMAGE3_ITEMS      # the cases of the range passes
        assert 7 < tok_id_range_lap(cu) + 5 < n - 1 and tok_range_lap(cu) + 5 < n


# ---------------------------------------------------------------- the lap batch ----

def lap_batch(W, V, K=KINDS):
    """Query q of a capped launch of W waves goes to wave j = q mod W on lap q // W.  -> (kind, variant), int64 arrays over the
    3 W + 37 queries of three full laps and 37 queries of a fourth: the query of wave j has kind j mod K on lap 0, (j / K) mod K
    on lap 1 and (j / K^2 + j) mod K on lap 2 -- so every ordered pair of kinds meets as (lap 0, lap 1) and as (lap 1, lap 2) of
    some wave as soon as W >= K^2 (the digit j / K^2 alone would need W >= K^3: a machine of one CU has 64 waves) -- and
    (j + 3) mod K on the fourth; its variant is (7 j + lap) mod V."""
    j = np.arange(W, dtype=np.int64)
    t = np.arange(TAIL, dtype=np.int64)
    kind = np.concatenate((j % K, (j // K) % K, (j // (K * K) + j) % K, (t + 3) % K))
    variant = np.concatenate([(7 * j + lap) % V for lap in range(LAPS)] + [(7 * t + LAPS) % V])
    return kind, variant


def pairs_met(kind, W, K, lap):
    """the set of (kind on `lap`, kind on `lap` + 1) over the waves"""
    a, b = kind[lap * W:(lap + 1) * W], kind[(lap + 1) * W:(lap + 2) * W]
    return set(zip(a.tolist(), b.tolist()))


@pytest.mark.parametrize("W", [64, 512, 16384])
def test_lap_batch_meets_every_ordered_pair_of_kinds(W):
    for V in (1, 3, 4, 5):
        kind, variant = lap_batch(W, V)
        assert kind.size == variant.size == LAPS * W + TAIL
        assert int(kind.min()) == 0 and int(kind.max()) == KINDS - 1 and int(variant.min()) == 0 and int(variant.max()) == V - 1
        every = {(a, b) for a in range(KINDS) for b in range(KINDS)}
        assert pairs_met(kind, W, KINDS, 0) == every and pairs_met(kind, W, KINDS, 1) == every
        q = np.arange(kind.size)
        assert np.array_equal(variant, (7 * (q % W) + q // W) % V)
        assert np.array_equal(kind[:W], np.arange(W) % KINDS) and np.array_equal(kind[W:2 * W], (np.arange(W) // KINDS) % KINDS)
        assert set(kind[LAPS * W:].tolist()) == set(range(KINDS))                      # the fourth lap has every kind as well
        if V > 1 and W % V:                                                           # a wave meets another variant on its next lap
            assert np.any(variant[:W] != variant[W:2 * W])


@pytest.mark.parametrize("W", [128, 16384])
def test_lap_batch_of_ten_kinds(W):
    kind, variant = lap_batch(W, 3, 10)
    every = {(a, b) for a in range(10) for b in range(10)}
    assert kind.size == LAPS * W + TAIL and pairs_met(kind, W, 10, 0) == every and pairs_met(kind, W, 10, 1) == every


# ---------------------------------------------------------------- from distinct queries to the batch ----

def pool_of(rows, dtype):
    """rows: one 1-D array per distinct query -> (off, data): the rows behind one another and their offsets"""
    rows = [np.asarray(r, dtype=dtype).reshape(-1) for r in rows]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.size for r in rows])
    return off, (np.concatenate(rows) if off[-1] else np.zeros(0, dtype=dtype))


def gather(pool_off, pool_data, ids):
    """the rows ids[0], ids[1], ... of a pool behind one another -> (off, data), off: len(ids) + 1 offsets.  numpy indexing only:
    a batch of tens of thousands of queries is assembled from the few distinct ones without a Python loop over it."""
    ids = np.asarray(ids, dtype=np.int64)
    lens = (pool_off[1:] - pool_off[:-1])[ids]
    off = np.zeros(ids.size + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    shift = np.repeat(pool_off[:-1][ids] - off[:-1], lens)
    idx = np.arange(off[-1], dtype=np.int64) + shift
    return off, (pool_data[idx] if off[-1] else pool_data[:0].copy())


def test_gather_is_the_concatenation():
    rng = np.random.default_rng(3)
    rows = [rng.integers(0, 1000, int(k)) for k in (0, 1, 5, 0, 300, 2, 64)]
    off, data = pool_of(rows, np.uint16)
    assert off.tolist() == [0, 0, 1, 6, 6, 306, 308, 372] and data.dtype == np.uint16
    for ids in ([], [0], [3, 0, 3], [4, 4, 1, 6, 0, 2, 5, 4], rng.integers(0, 7, 1000).tolist()):
        goff, got = gather(off, data, ids)
        want = [rows[i] for i in ids]
        assert goff.tolist() == np.concatenate(([0], np.cumsum([w.size for w in want]))).astype(np.int64).tolist()
        assert got.dtype == np.uint16 and got.tolist() == [int(x) for w in want for x in w]


# ---------------------------------------------------------------- the back-off as a probe-counting model ----

def backoff_model(cap, count_of, min_count):
    """the bisection of k_infgram_suffix on the suffix length: good = 0 always qualifies, bad = cap + 1 never does, one range
    search per probe of s = good + (bad - good) / 2.  count_of(s): the occurrences of the suffix of s symbols -> (s, probes)"""
    good, bad, probes = 0, cap + 1, 0
    while bad - good > 1:
        s = good + (bad - good) // 2
        probes += 1
        if count_of(s) >= min_count:
            good = s
        else:
            bad = s
    return good, probes


def test_backoff_model_is_both_definitions(oracle):
    """the byte definition counts its probes itself; the token definition tries every length, longest first"""
    tb = b"abracadabra abracadabra cadabra"
    arr = oracle.sais(np.frombuffer(tb, dtype=np.uint8))
    t = list(tb)
    tarr = tokens_abi.brute_suffix_array(t).tolist()
    assert tarr == arr.tolist()
    for prompt in (b"", b"x", b"cadabra", b"xcadabra", b"abrax", tb, b"q" + tb, b"a a a a a a a a"):
        for min_count, max_len in ((1, 0), (2, 0), (3, 4), (4, 1), (len(tb) + 2, 0)):
            L = len(prompt)
            cap = ngram_abi.backoff_cap(L, max_len)

            def count_of(s):
                lo, hi = ngram_abi.range_definition(tb, arr, prompt[L - s:])
                return hi - lo
            s, probes = backoff_model(cap, count_of, min_count)
            want = ngram_abi.infgram_definition(tb, arr, prompt, min_count, max_len)
            assert (s, probes) == (want[0], want[5]) and probes <= ngram_abi.ceil_log2(cap + 1)
            assert s == tokens_abi.infgram_definition(t, tarr, list(prompt), min_count, max_len)[0]
