"""Seeded synthetic corpora (ctypes binding of csrc/textgen.c) for BASELINE.json's configs.

C1/C2/C5 uniform bytes, C3 English-like Zipf word model, C4 DNA-like sigma=4 -- the offline
analogues of the reference's benchmark data (reference benches/utils.rs:17-45, :206-210).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def _gen():
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "libsa_textgen.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: run __graft_entry__.build()")
        L = ctypes.CDLL(path)
        L.sa_gen_uniform.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64]
        L.sa_gen_sigma.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32]
        L.sa_gen_dna.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64]
        L.sa_gen_dna_repeats.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double]
        L.sa_gen_english.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32]
        L.sa_gen_english.restype = ctypes.c_int32
        L.sa_gen_english_corpus.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_double]
        L.sa_gen_english_corpus.restype = ctypes.c_int32
        _lib = L
    return _lib


def uniform(n: int, seed: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    _gen().sa_gen_uniform(out.ctypes.data, n, seed)
    return out


def sigma(n: int, seed: int, sigma: int, base: int = 0) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    _gen().sa_gen_sigma(out.ctypes.data, n, seed, sigma, base)
    return out


def dna(n: int, seed: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    _gen().sa_gen_dna(out.ctypes.data, n, seed)
    return out


def dna_repeats(n: int, seed: int, fraction: float = 0.2) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    _gen().sa_gen_dna_repeats(out.ctypes.data, n, seed, fraction)
    return out


def english(n: int, seed: int, vocab: int = 50000) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    rc = _gen().sa_gen_english(out.ctypes.data, n, seed, vocab)
    if rc:
        raise MemoryError("sa_gen_english")
    return out


def english_iid(n: int, seed: int, vocab: int = 50000) -> np.ndarray:
    """round-1 C3 model: iid Zipf words, no phrase reuse (mean LCP 9, max 29 at 32 MiB) -- kept as `c3_iid_256m`"""
    return english(n, seed, vocab)


def english_corpus(n: int, seed: int, vocab: int = 50000, dup_fraction: float = 0.08) -> np.ndarray:
    """C3: English-like text with the repeat structure of a real corpus (word bigrams, stock sentences, copied passages
    with mutations; csrc/textgen.c sa_gen_english_corpus) -- the offline stand-in for Pizza&Chili `english`
    (reference benches/utils.rs:24-45)"""
    out = np.empty(n, dtype=np.uint8)
    rc = _gen().sa_gen_english_corpus(out.ctypes.data, n, seed, vocab, dup_fraction)
    if rc:
        raise MemoryError("sa_gen_english_corpus")
    return out


def _zipf_text(rng, ids: np.ndarray, n: int) -> np.ndarray:
    """n draws of ids[rank], rank Zipf-distributed (weight 1 / rank), then one block of n / 16 entries repeated further on"""
    vocab = ids.size
    cdf = np.cumsum(1.0 / np.arange(1, vocab + 1, dtype=np.float64))
    out = np.empty(n, dtype=ids.dtype)
    step = 1 << 22
    for a in range(0, n, step):                                   # in pieces: the float64 draws of 128 Mi tokens would be 1 GiB
        b = min(n, a + step)
        out[a:b] = ids[np.minimum(np.searchsorted(cdf, rng.random(b - a) * cdf[-1]), vocab - 1)]
    blk = n // 16
    if blk:
        src = int(rng.integers(0, n - 2 * blk + 1))
        dst = int(rng.integers(src + blk, n - blk + 1))
        out[dst:dst + blk] = out[src:src + blk]
    return out


def token_corpus(n: int, vocab: int = 50000, seed: int = 0) -> np.ndarray:
    """n tokeniser-like ids (uint16) for the 16-bit token texts: Zipf-distributed ranks (weight 1 / rank) over `vocab` <= 65 536
    words, the rank -> id map a seeded permutation (frequent words get ids with any high byte), and one block of n / 16 tokens
    repeated further on (a copied passage: long common prefixes).  numpy only; the same array for the same arguments."""
    if not 1 <= vocab <= 65536:
        raise ValueError("token_corpus: 1 <= vocab <= 65536")
    rng = np.random.default_rng([int(seed), int(vocab), 0x746F6B])
    return _zipf_text(rng, rng.permutation(vocab).astype(np.uint16), n)


def token_corpus_u32(n: int, vocab: int = 128000, seed: int = 0) -> np.ndarray:
    """n tokeniser-like ids (uint32, every id below 2^24) for the 32-bit token texts: the Zipf ranks and the copied passage of
    ``token_corpus`` over `vocab` <= 2^24 words.  The rank -> id map is the seeded bijection rank * a + b modulo 2^24 (a odd), so
    whatever the vocabulary the ids -- those of the frequent words too -- differ in each of their three bytes."""
    if not 1 <= vocab <= 1 << 24:
        raise ValueError("token_corpus_u32: 1 <= vocab <= 2**24")
    rng = np.random.default_rng([int(seed), int(vocab), 0x746F6B, 32])
    a, b = (int(x) for x in rng.integers(0, 1 << 24, 2))
    ids = ((np.arange(vocab, dtype=np.uint64) * np.uint64(a | 1) + np.uint64(b)) & np.uint64(0xFFFFFF)).astype(np.uint32)
    return _zipf_text(rng, ids, n)


#: BASELINE.md section 2 workloads: name -> (generator, n, seed)
WORKLOADS = {
    "c1_uniform_1k": (uniform, 1 << 10, 1),
    "c2_uniform_64m": (uniform, 64 << 20, 2),
    "c3_english_256m": (english_corpus, 256 << 20, 3),
    "c3_iid_256m": (english_iid, 256 << 20, 3),
    "c2_uniform_256m": (uniform, 256 << 20, 2),          # north_star's literal "256 MiB random-byte text"
    "c4_dna_1g": (dna, 1 << 30, 4),
    "c4_dna_repeats_1g": (lambda n, seed: dna_repeats(n, seed, 0.2), 1 << 30, 4),   # the harder C4 variant (planted repeats of 1-100 KiB, 1 % mutations)
    "c5_uniform_512m": (uniform, 512 << 20, 50),
}


def workload(name: str, rank: int = 0, n_override: int | None = None) -> np.ndarray:
    gen, n, seed = WORKLOADS[name]
    return gen(n_override if n_override is not None else n, seed + rank)
