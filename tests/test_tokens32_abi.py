"""CPU suite for the 32-bit token texts, ids below 2^24 (kernels/tokens.hpp, host/tokens.hpp): the argument
for the construction route (the suffix array of the big-endian image at THREE bytes a token, its entries divisible by 3 divided by
3 -- and neither the little-endian image nor the 16-bit form on truncated ids), a model of the compaction at stride 3, the one
multiply that is its test and its quotient, a model of the group compare at one token a word, the header's example, the exports,
the Python surface and the argument checks that answer without a device.  The width-agnostic definitions come from
tests/test_tokens_abi.py and tests/test_tok_score_abi.py unchanged; tests/test_tokens32.py imports the text families from here."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import MAX_TOKENS_U32, TOKEN_LIMIT_U32, TokenIndex32, corpus, saca_u32
from suffix_array_amd.corpus import token_corpus_u32
from conftest import ROOT
from test_tok_score_abi import NAMES, score_definition
from test_tokens_abi import (BRUTE_MAX, SPAN, TILE, brute_suffix_array, compaction_model, fibonacci_tokens, infgram_definition,
                             next_tokens_definition, range_definition)

EXPORTS = ("sa_amd_max_tokens_u32", "sa_amd_saca_u32", "sa_amd_tok32_index_create", "sa_amd_tok32_index_destroy", "sa_amd_tok32_index_sa",
           "sa_amd_tok32_index_search", "sa_amd_tok32_index_next_tokens", "sa_amd_tok32_index_infgram", "sa_amd_tok32_index_infgram_score")
EXAMPLE_TEXT = [65537, 1, 65536, 1, 2]
EXAMPLE_SA = [5, 3, 1, 4, 2, 0]
EXAMPLE_TRUNCATED_SA = [5, 2, 1, 0, 3, 4]                             # of the ids & 0xFFFF = {1, 1, 0, 1, 2}
EXAMPLE_QUERY = [7, 65536, 1, 2]
LIMIT = 1 << 24
GROUP = 8                                                             # SCORE_G: lanes that serve one position
ERANGE, EINVAL = -6, -1


# ---------------------------------------------------------------- the route ----

def as_tokens32(t):
    return np.ascontiguousarray(t, dtype=np.uint32)


def be_image3(tokens):
    """B[3 i], B[3 i + 1], B[3 i + 2] = the three bytes of token i, the top one first"""
    t = as_tokens32(tokens)
    assert t.size == 0 or int(t.max()) < LIMIT
    return t.astype(">u4").view(np.uint8).reshape(-1, 4)[:, 1:].reshape(-1).copy()


def le_image3(tokens):
    t = as_tokens32(tokens)
    return t.astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


def every_third_thirded(byte_sa):
    a = np.asarray(byte_sa, dtype=np.uint32)
    return (a[a % 3 == 0] // 3).astype(np.uint32)


def reference_suffix_array32(tokens, oracle):
    """brute force where it is affordable, else the route this suite pins: the oracle on the 3-byte big-endian image"""
    if len(tokens) <= BRUTE_MAX:
        return brute_suffix_array(tokens)
    return every_third_thirded(oracle.sais(be_image3(tokens)))


def families32(n, seed=0):
    """name -> n tokens below 2^24; every family the construction is tested on"""
    rng = np.random.default_rng(seed + 11 * n)
    out = {
        "one_token": np.full(n, 0x010000),
        "period_3": np.resize(np.array([0x010000, 0x000100, 0x000001]), n),
        "below_256": rng.integers(0, 256, n),
        "multiples_of_65536": rng.integers(0, 256, n) * 65536,
        "top_byte_only": rng.integers(0, 256, n) * 65536 + 0x00ABCD,
        "zeros_and_ffffff": np.where(rng.random(n) < 0.5, 0x000000, 0xFFFFFF),
        "fibonacci": np.array(fibonacci_tokens(n, 1, 65536), dtype=np.int64) if n else np.zeros(0, dtype=np.int64),
        "zipf_200000": token_corpus_u32(n, 200000, seed + 1),
    }
    return {k: as_tokens32(v) for k, v in out.items()}


SMALL_SIZES = (0, 1, 2, 3, 5, 64, 65, 257, 700)


def small_cases32():
    yield "header", as_tokens32(EXAMPLE_TEXT)
    for n in SMALL_SIZES:
        for name, t in families32(n).items():
            yield f"{name}_{n}", t


def test_header_example_is_the_brute_force_array():
    assert brute_suffix_array(EXAMPLE_TEXT).tolist() == EXAMPLE_SA
    assert brute_suffix_array([x & 0xFFFF for x in EXAMPLE_TEXT]).tolist() == EXAMPLE_TRUNCATED_SA != EXAMPLE_SA


def test_three_byte_image_route_gives_the_token_order(oracle):
    """oracle.sais of the 3-byte big-endian image, filtered to the entries divisible by 3 and divided by 3, is the brute-force
    array on every case: 3 n + 1 entries in, n + 1 out, the entry 3 n first"""
    seen = 0
    for name, t in small_cases32():
        image = be_image3(t)
        assert image.size == 3 * t.size
        byte_sa = oracle.sais(image)
        assert byte_sa.size == 3 * t.size + 1
        got = every_third_thirded(byte_sa)
        assert got.size == t.size + 1 and got[0] == t.size, name
        assert np.array_equal(got, brute_suffix_array(t)), name
        seen += 1
    assert seen == 1 + len(SMALL_SIZES) * 8


def test_neither_the_little_endian_image_nor_truncation_does(oracle):
    """the negative checks, on the header example: the little-endian image gives another order, and so does the 16-bit form on the
    ids truncated to 16 bits -- a test that passes with either shows nothing, this text tells them apart"""
    t = as_tokens32(EXAMPLE_TEXT)
    got = every_third_thirded(oracle.sais(le_image3(t)))
    assert got.size == t.size + 1 and got.tolist() != EXAMPLE_SA
    t16 = (t & 0xFFFF).astype(">u2").view(np.uint8)
    byte_sa = oracle.sais(t16.copy())
    truncated = (byte_sa[(byte_sa & 1) == 0] >> 1).tolist()
    assert truncated == EXAMPLE_TRUNCATED_SA and truncated != EXAMPLE_SA
    assert every_third_thirded(oracle.sais(be_image3(t))).tolist() == EXAMPLE_SA


def test_image_bytes():
    assert be_image3([0x123456, 0x0000FF, 0xFF0000]).tolist() == [0x12, 0x34, 0x56, 0, 0, 0xFF, 0xFF, 0, 0]
    assert le_image3([0x123456]).tolist() == [0x56, 0x34, 0x12]
    assert be_image3([]).size == 0


def test_token_corpus_u32_is_seeded_zipf_and_reaches_every_byte():
    a, b = token_corpus_u32(5000, 200000, 3), token_corpus_u32(5000, 200000, 3)
    assert a.dtype == np.uint32 and a.shape == (5000,) and np.array_equal(a, b)
    assert not np.array_equal(a, token_corpus_u32(5000, 200000, 4))
    assert int(a.max()) < LIMIT and np.unique(a).size > 1000
    for shift in (0, 8, 16):                                          # every byte of the 24 bits varies, the top one too
        assert np.unique((a >> shift) & 255).size > 200, shift
    counts = np.sort(np.bincount(np.unique(a, return_inverse=True)[1]))[::-1]
    assert counts[0] > 20 * np.median(counts)                         # Zipf: a head far above the typical word
    assert token_corpus_u32(0, 10, 1).size == 0 and np.unique(token_corpus_u32(4000, 100, 1)).size <= 100
    blk = 5000 // 16                                                  # the copied passage: one block occurs twice
    windows = {a[i:i + blk].tobytes() for i in range(0, 5000 - blk + 1)}
    assert len(windows) < 5000 - blk + 1
    assert token_corpus_u32(16, 1 << 24, 1).size == 16
    for vocab in (0, (1 << 24) + 1):
        with pytest.raises(ValueError):
            token_corpus_u32(10, vocab, 1)
    assert np.array_equal(corpus.token_corpus(300, 50000, 3), corpus.token_corpus(300, 50000, 3))
    assert corpus.token_corpus(300, 50000, 3).dtype == np.uint16      # the 16-bit generator is what it was


# ---------------------------------------------------------------- the compaction at stride 3 ----

def kept_by_multiply(e):
    """tok_kept<3> of kernels/tokens.hpp: q = e * 0xAAAAAAAB modulo 2^32; e is divisible by 3 iff q <= 0x55555555, and then q = e / 3"""
    q = (np.asarray(e, dtype=np.uint64) * np.uint64(0xAAAAAAAB)) & np.uint64(0xFFFFFFFF)
    return q <= np.uint64(0x55555555), q.astype(np.uint32)


def test_the_multiply_is_the_test_and_the_quotient():
    assert (3 * 0xAAAAAAAB) % (1 << 32) == 1 and 0x55555555 == (2**32 - 1) // 3
    rng = np.random.default_rng(3)
    samples = [np.arange(1 << 16, dtype=np.uint64), np.arange((1 << 24) - 4096, (1 << 24) + 4096, dtype=np.uint64),
               rng.integers(0, 1 << 31, 1 << 18).astype(np.uint64), np.arange(2**31 - 4096, 2**31, dtype=np.uint64),
               np.arange(2**32 - 4096, 2**32, dtype=np.uint64), np.array([0, 1, 2, 3, 3 * 715827882, 3 * 715827882 + 1], dtype=np.uint64)]
    for e in samples:
        keep, q = kept_by_multiply(e)
        assert np.array_equal(keep, e % 3 == 0)
        assert np.array_equal(q[keep].astype(np.uint64), e[keep] // 3)
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "tokens.hpp")) as f:
        src = f.read()
    assert "*q = e * 0xAAAAAAABu; return *q <= 0x55555555u;" in src


def compaction_model_stride(byte_sa, stride, tile=TILE, span=SPAN):
    """compaction_model of tests/test_tokens_abi.py with the kept test and the quotient of `stride`: per tile the number of kept
    entries, an exclusive scan over tiles + 1 words, then per tile the kept entries, divided, at the tile's offset plus their rank"""
    a = np.asarray(byte_sa, dtype=np.uint32)
    if stride == 3:
        keep_all, quot = kept_by_multiply(a)
    else:
        keep_all, quot = (a & 1) == 0, a >> 1
    tiles = -(-a.size // tile)
    cnt = np.zeros(tiles + 1, dtype=np.int64)
    for sp in range(-(-tiles // span)):
        for k in range(span):
            tl = sp * span + k
            if tl < tiles:
                cnt[tl] = int(np.count_nonzero(keep_all[tl * tile:(tl + 1) * tile]))
    off = np.concatenate(([0], np.cumsum(cnt)[:-1]))
    out = np.full(int(off[tiles]), 0xFFFFFFFF, dtype=np.uint32)
    for tl in range(tiles):
        keep = keep_all[tl * tile:(tl + 1) * tile]
        rank = np.cumsum(keep) - keep
        out[off[tl] + rank[keep]] = quot[tl * tile:(tl + 1) * tile][keep]
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 682, 683, 2730, 2731, 3 * 2731 + 77])
def test_stride_3_compaction_model_is_the_filter(n):
    """3 n + 1 on either side of one tile (n = 682: 2047, n = 683: 2050) and of one span of four tiles (n = 2730: 8191, 2731: 8194)"""
    assert (3 * 682 + 1 < TILE < 3 * 683 + 1) and (3 * 2730 + 1 < SPAN * TILE < 3 * 2731 + 1)
    rng = np.random.default_rng(n)
    byte_sa = rng.permutation(3 * n + 1).astype(np.uint32)            # any arrangement of 0 .. 3 n: n + 1 entries divisible by 3
    got = compaction_model_stride(byte_sa, 3)
    assert got.size == n + 1 and np.array_equal(got, every_third_thirded(byte_sa))
    assert np.array_equal(compaction_model_stride(byte_sa, 3, 64, 3), got)
    even = rng.permutation(2 * n + 1).astype(np.uint32)               # the generic model at stride 2 is the 16-bit suite's model
    assert np.array_equal(compaction_model_stride(even, 2), compaction_model(even))


def test_the_compaction_is_one_template_over_the_stride():
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "tokens.hpp")) as f:
        src = f.read()
    for name in ("tok_compact_load", "k_tok_compact_count", "k_tok_compact_scatter"):
        assert len(re.findall(r"\b" + name + r"\(const uint32_t \*__restrict__ SA2", src)) == 1, name      # one definition each
        assert re.search(r"template <int STRIDE>\s+__(global|device)__[^;{]*\b" + name + r"\(", src), name
    assert src.count("__ballot((keep[c] >> k) & 1u)") == 1            # the rank code of the scatter stands once


# ---------------------------------------------------------------- the group compare at one token a word ----

def group_compare_model32(text, pat, frm, limit, lanes=GROUP):
    """match_group_lcp<G, uint32_t> of kernels/match.hpp, after group_compare_model of tests/test_tok_score_abi.py: W = 1, lane gl
    compares the word -- the token -- at offset off + gl, no word has a partial tail, the first differing lane is found and the
    order is that of the two 32-bit VALUES.  -> (lcp, less, tokens charged)"""
    charged = 0
    off = frm
    while off < limit:
        found = None
        for gl in range(lanes):
            o = off + gl
            if o >= limit:
                continue
            tw, qw = text[o] if o < len(text) else 0, pat[o] if o < len(pat) else 0
            if (tw ^ qw) and found is None:
                found = (gl, tw, qw)
        charged += lanes
        if found:
            gl, tw, qw = found
            return off + gl, tw < qw, charged
        off += lanes
    return limit, False, charged


def list_compare(text, pat, limit):
    lcp = next((i for i in range(limit) if text[i] != pat[i]), limit)
    return lcp, (lcp < limit and text[lcp] < pat[lcp])


def test_word_compare_model_at_one_token_a_word():
    pairs = [(0x010203, 0x030201), (0x030201, 0x010203),              # every byte order crossed
             (0x010000, 0x00FFFF), (0x00FFFF, 0x010000),              # the top byte decides against both lower ones
             (0x0100AB, 0x0200AB), (0xFF00AB, 0x0000AB),              # differ only in the top byte
             (0x000001, 0x000002), (0x000000, 0xFFFFFF), (0xFFFFFF, 0x000000), (0x00FF00, 0x010000)]
    for a, b in pairs:
        for at in (0, 1, 7, 8, 9, 15, 16, 30):                        # the group's first and last lane, the next round
            for limit in (at + 1, at + 2, 40):
                base = [0x010101 * (i % 7 + 1) for i in range(limit)]
                text, pat = list(base), list(base)
                text[at], pat[at] = a, b
                text_x, pat_x = text + [0x111111, 0x222222], pat + [0x333333, 0x000001]      # garbage behind the limit must not show
                for frm in sorted({0, min(at, 1), at - at % GROUP, at}):
                    got = group_compare_model32(text_x, pat_x, frm, limit)
                    assert got[:2] == list_compare(text, pat, limit), (hex(a), hex(b), at, limit, frm)
                    assert got[2] % GROUP == 0 and got[2] >= GROUP
    assert group_compare_model32([5, 9], [5, 7], 0, 1) == (1, False, 8)
    assert group_compare_model32([5, 6], [5, 7], 0, 2) == (1, True, 8)
    assert group_compare_model32(list(range(40)), list(range(40)), 3, 36) == (36, False, 5 * 8)
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "match.hpp")) as f:
        src = f.read()
    assert "if constexpr (sizeof(Sym) == 4) {" in src and "*less = tw < qw;" in src
    assert "<< 32" not in src.replace("(uint64_t)w1 << 32", "").replace("(unsigned long long)ml << 32", "")      # no 32-bit shift by 32


# ---------------------------------------------------------------- the header's example and the definitions ----

def header_text(name="suffix_array_amd_tok32.h"):
    """the header that declares and documents the 32-bit token forms; include/suffix_array_amd.h includes it"""
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_the_header_example():
    t, arr = EXAMPLE_TEXT, EXAMPLE_SA
    rows = {(65536, 1): (4, 5, 0, [(2, 1)]), (1,): (1, 3, 0, [(2, 1), (65536, 1)]), (2,): (3, 4, 1, []),
            (): (0, 6, 1, [(1, 2), (2, 1), (65536, 1), (65537, 1)])}
    for ctx, want in rows.items():
        assert next_tokens_definition(t, arr, list(ctx)) == want, ctx
    lo, hi, ae, listing = next_tokens_definition(t, arr, [9])
    assert lo == hi and ae == 0 and listing == []
    prompt = [7, 65536, 1]
    assert infgram_definition(t, arr, prompt, 1, 0)[:3] == (2, 4, 5)
    assert infgram_definition(t, arr, prompt, 2, 0)[:3] == (1, 1, 3)
    assert infgram_definition(t, arr, prompt, 3, 0)[:3] == (0, 0, 6)
    raw = header_text()
    header = re.sub(r"\s+", " ", raw).replace(" * ", " ")
    for row in ("T = {65537, 1, 65536, 1, 2}, SA = {5, 3, 1, 4, 2, 0}.", "the ids are {1, 1, 0, 1, 2}, whose array is {5, 2, 1, 0, 3, 4}",
                "{65536, 1} [4, 5) 0 {2:1}", "{1} [1, 3) 0 {2:1, 65536:1}", "{2} [3, 4) 1 empty",
                "{} [0, 6) 1 {1:2, 2:1, 65536:1, 65537:1}", "{9} empty 0 empty", "{7, 65536, 1} 1 none 2 [4, 5)",
                "{7, 65536, 1} 2 none 1 [1, 3)", "{7, 65536, 1} 3 none 0 [0, 6)"):
        assert row in header, row
    d = score_definition(t, arr, EXAMPLE_QUERY, None, 1, 4)
    assert "Q = {7, 65536, 1, 2}, one document, min_count = 1, max_len = 4 (sa_amd_tok32_index_infgram_score):" in raw
    block = raw[raw.index("Q = {7, 65536, 1, 2}"):]
    for j, q in enumerate(EXAMPLE_QUERY):                             # every line rebuilt from the definition
        s, lo, hi, ae, nlo, nhi = (int(d[k][j]) for k in NAMES)
        line = f" *     {j}  {q:<5d}  {s}  " + f"[{lo}, {hi})".ljust(10) + f"{ae}       [{nlo}, {nhi})\n"
        assert line in block, line


def contexts_of32(t, rng):
    n = len(t)
    out = [[], [9], [LIMIT - 1], [0], [65536]]
    for _ in range(10):
        if n:
            a = int(rng.integers(0, n))
            k = int(rng.integers(1, 6))
            out.append(t[a:a + k])
            out.append(t[a:a + k] + [int(rng.integers(0, LIMIT))])
            piece = t[a:a + k]
            out.append(piece[:-1] + [piece[-1] ^ 0x010000])            # differs in the top byte of its last token
    out += [t[max(n - 2, 0):], list(t), list(t) + [1]]
    return out


def test_the_definitions_hold_at_24_bits():
    """the imported definitions are width-agnostic: on texts with ids above 65 535 their listings imply the sub-range identity"""
    rng = np.random.default_rng(5)
    for name, tok in small_cases32():
        if tok.size > 70:
            continue
        t = [int(x) for x in tok]
        arr = brute_suffix_array(t).tolist()
        for ctx in contexts_of32(t, rng):
            lo, hi, ae, listing = next_tokens_definition(t, arr, ctx)
            at = lo + ae
            for v, c in listing:
                assert range_definition(t, arr, ctx + [v]) == (at, at + c), (name, ctx[:8], v)
                at += c
            assert at == hi


# ---------------------------------------------------------------- the surface ----

def declarations(name="suffix_array_amd_tok32.h"):
    plain = re.sub(r"/\*.*?\*/", " ", header_text(name), flags=re.S)
    return {name: [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
            for name, params in re.findall(r"\b(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", plain)}


def test_header_declares_and_library_exports_the_entry_points():
    header = header_text()
    decls = declarations()
    L = ctypes.CDLL(sa.library_path())
    assert set(decls) == set(EXPORTS)                                 # what the file declares is what this suite and tests/test_tokens32.py cover
    for fn in EXPORTS:
        assert hasattr(L, fn), fn
        assert not any("stream" in p for p in decls[fn]), fn         # host pointers only: no device form, no stream
    assert not any(name.endswith("_device") for name in decls)
    main = header_text("suffix_array_amd.h")                          # one interface: the main header brings these declarations in
    assert re.search(r'^#include "suffix_array_amd_tok32.h"$', main, re.M) and re.search(r'^#include "suffix_array_amd.h"$', header, re.M)
    probe = "#include \"suffix_array_amd.h\"\nint32_t (*probe)(const uint32_t *, uint32_t *, int32_t) = sa_amd_saca_u32;\n"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=probe.encode(), check=True)
    decls.update(declarations("suffix_array_amd.h"))
    assert re.search(r"^#define SA_AMD_TOKEN_LIMIT_U32 \(1 << 24\)$", header, re.M)
    L.sa_amd_max_tokens_u32.restype = ctypes.c_int32
    assert L.sa_amd_max_tokens_u32() == MAX_TOKENS_U32 == sa.MAX_TOKENS_U32 == (2**31 - 1) // 3 == 715827882
    assert TOKEN_LIMIT_U32 == sa.TOKEN_LIMIT_U32 == LIMIT
    # the signatures are the u16 ones with uint32_t tokens and the other handle
    pairs = [("sa_amd_saca_u16", "sa_amd_saca_u32")] + [("sa_amd_tok_index_" + op, "sa_amd_tok32_index_" + op)
                                                      for op in ("create", "destroy", "sa", "search", "next_tokens", "infgram", "infgram_score")]
    for narrow, wide in pairs:
        want = [p.replace("sa_amd_tok_index", "sa_amd_tok32_index").replace("uint16_t", "uint32_t") for p in decls[narrow]]
        assert decls[wide] == want, wide
    with open(os.path.join(ROOT, "include", "suffix_array_amd.hpp")) as f:
        hpp = f.read()
    assert "using TokenIndex32 = BasicTokenIndex<TokenAbi32>;" in hpp and "using TokenIndex = BasicTokenIndex<TokenAbi16>;" in hpp


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for name in ("saca_u32", "MAX_TOKENS_U32", "TOKEN_LIMIT_U32", "TokenIndex32"):
        assert name in sa.__all__ and hasattr(sa, name), name
    assert sa.saca_u32 is saca_u32 and sa.TokenIndex32 is TokenIndex32
    assert params(saca_u32) == ["tokens"] and params(TokenIndex32.__init__) == ["self", "tokens", "sa"]
    assert inspect.signature(TokenIndex32.__init__).parameters["sa"].default is None
    for op in ("sa", "search", "count", "contains", "next_tokens", "infgram", "infgram_score"):
        assert callable(getattr(TokenIndex32, op)), op
        assert params(getattr(TokenIndex32, op)) == params(getattr(sa.TokenIndex, op)), op
    assert [inspect.signature(TokenIndex32.infgram).parameters[k].default for k in ("min_count", "max_len")] == [1, 0]
    assert params(corpus.token_corpus_u32) == ["n", "vocab", "seed"] and params(corpus.token_corpus) == ["n", "vocab", "seed"]


BAD_TOKENS = (([1, 2**24], ValueError), ([-1], ValueError), ([1.5], TypeError), (["a"], TypeError), (b"ab", TypeError), ("ab", TypeError),
              (np.zeros(3, dtype=np.uint16), TypeError), (np.zeros(3, dtype=np.int64), TypeError), (np.zeros(3, dtype=np.int32), TypeError),
              (np.zeros((2, 2), dtype=np.uint32), TypeError), ([True], TypeError))


def test_python_rejects_bad_tokens_before_the_library_is_called(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sa, "lib", no_library)
    ix = object.__new__(TokenIndex32)
    for bad, err in BAD_TOKENS:
        with pytest.raises(err):
            saca_u32(bad)
        with pytest.raises(err):
            TokenIndex32(bad)
        with pytest.raises(err):
            sa._token_batch32([[1, 2], bad])
        for call in (ix.search, ix.count, ix.contains, ix.next_tokens, ix.infgram):
            with pytest.raises(err):
                call([[1, 2], bad])
        with pytest.raises(err):
            ix.infgram_score(bad)
    over = np.array([1, 2**24], dtype=np.uint32)                      # an array is a pattern's ids too: checked here, never uploaded
    for call in (ix.search, ix.next_tokens, ix.infgram):
        with pytest.raises(ValueError):
            call([over])
    with pytest.raises(ValueError):
        ix.infgram_score(over)
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram([[1]], min_count=0)
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score([1, 2], min_count=0)
    data, off, cnt = sa._token_batch32([[1, 2], np.array([2**24 - 1], dtype=np.uint32), []])
    assert data.dtype == np.uint32 and data.tolist() == [1, 2, 2**24 - 1] and off.tolist() == [0, 2, 3, 3] and cnt == 3
    data, off, cnt = sa._token_batch32([])
    assert data.size >= 1 and off.tolist() == [0] and cnt == 0


def test_the_16_bit_forms_reject_what_they_rejected(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sa, "lib", no_library)
    for bad, err in (([1, 65536], ValueError), (np.zeros(3, dtype=np.uint32), TypeError), ([-1], ValueError)):
        with pytest.raises(err):
            sa.saca_u16(bad)
        with pytest.raises(err):
            sa.TokenIndex(bad)


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x00777777, dtype=np.uint32)                    # (as patterns: ids below 2^24)
    p = buf.ctypes.data
    tot = ctypes.c_int64(-5)
    c = ctypes.byref(tot)
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    bad = [np.array([0, 3, 2], dtype=np.int64), np.array([-1, 2, 4], dtype=np.int64), np.array([0, 2, -4], dtype=np.int64)]
    g = good.ctypes.data
    before = (sa.last_tok_stats(), sa.last_tok_score_stats())

    def score(ix, q, m, off, ndocs, min_count, max_len):
        return L.sa_amd_tok32_index_infgram_score(ix, q, m, off, ndocs, min_count, max_len, p, p, p, p, p, p)
    assert L.sa_amd_tok32_index_search(None, p, g, 2, p, p, p) == EINVAL                               # NULL index
    assert L.sa_amd_tok32_index_next_tokens(None, p, g, 2, p, p, p, p, p, p, 4, c) == EINVAL
    assert L.sa_amd_tok32_index_infgram(None, p, g, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == EINVAL
    assert score(None, p, 4, g, 2, 1, 8) == EINVAL and score(None, p, 0, None, 0, 1, 8) == EINVAL
    assert L.sa_amd_tok32_index_sa(None, p) == EINVAL and L.sa_amd_tok32_index_sa(fake, None) == EINVAL
    assert L.sa_amd_tok32_index_search(fake, p, g, -1, p, p, p) == EINVAL                              # negative count, capacity
    assert L.sa_amd_tok32_index_next_tokens(fake, p, g, -1, p, p, p, p, p, p, 4, c) == EINVAL
    assert L.sa_amd_tok32_index_next_tokens(fake, p, g, 2, p, p, p, p, p, p, -1, c) == EINVAL
    assert L.sa_amd_tok32_index_infgram(fake, p, g, -1, 1, 0, p, p, p, p, p, p, p, 4, c) == EINVAL
    assert L.sa_amd_tok32_index_infgram(fake, p, g, 2, 1, 0, p, p, p, p, p, p, p, -1, c) == EINVAL
    for min_count in (0, -1, -2**31):                                                                  # min_count < 1
        assert L.sa_amd_tok32_index_infgram(fake, p, g, 2, min_count, 0, p, p, p, p, p, p, p, 4, c) == EINVAL
        assert score(fake, p, 4, g, 2, min_count, 8) == EINVAL
    assert L.sa_amd_tok32_index_next_tokens(fake, p, None, 2, p, p, p, p, p, p, 4, c) == EINVAL        # pat_off as the search rejects it
    assert L.sa_amd_tok32_index_next_tokens(fake, None, g, 2, p, p, p, p, p, p, 4, c) == EINVAL
    for off in bad:
        assert L.sa_amd_tok32_index_search(fake, p, off.ctypes.data, 2, p, p, p) == EINVAL
        assert L.sa_amd_tok32_index_next_tokens(fake, p, off.ctypes.data, 2, p, p, p, p, p, p, 4, c) == EINVAL
        assert L.sa_amd_tok32_index_infgram(fake, p, off.ctypes.data, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == EINVAL
    assert score(fake, p, -1, None, 0, 1, 8) == EINVAL and score(fake, None, 4, None, 0, 1, 8) == EINVAL
    assert score(fake, p + 2, 4, None, 0, 1, 8) == EINVAL                                               # a query that is not 4-byte aligned
    for max_len in (0, -1, 4097, 2**31 - 1):
        assert score(fake, p, 4, g, 2, 1, max_len) == EINVAL
    for off in ([1, 2, 4], [0, 3, 2], [0, 2, 5]):
        assert score(fake, p, 4, np.array(off, dtype=np.int64).ctypes.data, 2, 1, 8) == EINVAL, off
    # a pattern, prompt or query id of 2^24: SA_AMD_ERANGE from the host scan, at every place of the batch, before the index is used
    for at in (0, 1, 3):
        pats = np.full(4, 5, dtype=np.uint32)
        pats[at] = 2**24
        q = pats.ctypes.data
        assert L.sa_amd_tok32_index_search(fake, q, g, 2, p, p, p) == ERANGE
        assert L.sa_amd_tok32_index_next_tokens(fake, q, g, 2, p, p, p, p, p, p, 4, c) == ERANGE
        assert L.sa_amd_tok32_index_infgram(fake, q, g, 2, 1, 0, p, p, p, p, p, p, p, 4, c) == ERANGE
        assert score(fake, q, 4, g, 2, 1, 8) == ERANGE and score(fake, q, 4, None, 0, 1, 8) == ERANGE
        pats[at] = 0xFFFFFFFF
        assert L.sa_amd_tok32_index_search(fake, q, g, 2, p, p, p) == ERANGE
    h = ctypes.c_void_p(p)
    for n in (-1, MAX_TOKENS_U32 + 1, sa.MAX_TOKENS_U16, 2**31 - 1):                                   # n < 0, n above the maximum
        assert L.sa_amd_saca_u32(p, p, n) == EINVAL
        assert L.sa_amd_tok32_index_create(p, n, None, ctypes.byref(h)) == EINVAL
    assert L.sa_amd_saca_u32(None, p, 3) == EINVAL and L.sa_amd_saca_u32(p, None, 3) == EINVAL and L.sa_amd_saca_u32(None, None, 0) == EINVAL
    assert L.sa_amd_tok32_index_create(None, 3, None, ctypes.byref(h)) == EINVAL and L.sa_amd_tok32_index_create(p, 3, None, None) == EINVAL
    assert tot.value == -5 and np.all(buf == 0x00777777)
    assert (sa.last_tok_stats(), sa.last_tok_score_stats()) == before
    one = np.full(3, 0x55555555, dtype=np.uint32)
    assert L.sa_amd_saca_u32(None, one.ctypes.data, 0) == 0 and one.tolist() == [0, 0x55555555, 0x55555555]      # n == 0: SA = {0}
    L.sa_amd_tok32_index_destroy(None)
    assert L.sa_amd_strerror(ERANGE)
