"""GPU suite for the LCP-accelerated search of the device index (-m gpu): DeviceIndex.enable_lcp builds the LCP table of the
search tree (kernels/esa.hpp k_esa_tree), later searches take the LCP route (k_esa_search).  Every answer equals the plain
route's and oracle/search_model.py's, in every order of buckets() and enable_lcp(); the text bytes compared stay within
2 plen + 128 log2 P (last_search_stats); the top of the range runs P = 2^31; SuffixArray.enable_lcp keeps its answers and
survives set()."""
import json
import os

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import adversarial_cases, fibonacci_word

import search_model
from test_lcp_search_abi import bound, log_p, plain_bytes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("contains", "lo", "hi", "lcp_start", "lcp_len")


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def _same(got, exp, pats, what):
    for k in KEYS:
        if not np.array_equal(got[k], exp[k]):
            bad = [q for q in range(len(pats)) if got[k][q] != exp[k][q]][:3]
            raise AssertionError(f"{what}: {k} differs at {[(bytes(pats[q][:40]), got[k][q], exp[k][q]) for q in bad]}")


def _patterns(rng, s, count, max_len=300):
    """cut from the text, half of them with one byte changed at a random depth, plus the edge cases"""
    n = len(s)
    out = [b"", s[:1], s[-1:], s, s + b"\x00", b"\xff" * 3, b"\x00", s[-200:]]
    while len(out) < count:
        if n == 0:
            out.append(bytes(rng.integers(0, 256, int(rng.integers(1, 4))).astype(np.uint8)))
            continue
        a = int(rng.integers(0, n))
        p = bytearray(s[a:a + int(rng.integers(1, max_len + 1))])
        if rng.random() < 0.5:
            k = int(rng.integers(0, len(p)))
            p[k] = (p[k] + int(rng.integers(1, 256))) & 0xFF
        out.append(bytes(p))
    return out


def _all_orders(text, arr, pats, model_pats=None, bkt=None):
    """plain route without / with the bucket table, then the LCP route with enable_lcp before, after and without buckets();
    model_pats (a subset) against search_model too"""
    ix = sa.DeviceIndex(text, arr)
    plain = ix.search(pats)
    assert sa.last_search_stats()["route"] == 0 and sa.last_search_stats()["compared_bytes"] == -1
    table = ix.buckets()
    plain_b = ix.search(pats)
    ix.close()
    if model_pats is not None:
        idx, mp = model_pats
        s = text
        _same({k: plain[k][idx] for k in KEYS}, search_model.search_many(s, arr, mp), mp, "plain vs model")
        _same({k: plain_b[k][idx] for k in KEYS}, search_model.search_many(s, arr, mp, table), mp, "plain+bkt vs model")
    ix = sa.DeviceIndex(text, arr)
    ix.enable_lcp()
    ix.enable_lcp()                                               # a no-op the second time
    _same(ix.search(pats), plain, pats, "lcp")
    st = sa.last_search_stats()
    assert st["route"] == 1 and st["patterns"] == len(pats) and st["steps"] == 2 * log_p(text.size) * len(pats)
    assert 0 <= st["table_steps"] <= st["steps"]
    assert np.array_equal(ix.buckets(), table)
    _same(ix.search(pats), plain_b, pats, "lcp, then buckets")
    ix.close()
    ix = sa.DeviceIndex(text, arr)
    ix.buckets()
    ix.enable_lcp()
    _same(ix.search(pats), plain_b, pats, "buckets, then lcp")
    ix.close()
    return st


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_adversarial_cases_every_order(oracle, name):
    s = adversarial_cases()[name]
    text = _u8(s)
    arr = oracle.sais(s)
    pats = _patterns(np.random.default_rng(len(s) + 5), s, 60, max_len=5000)
    _all_orders(text, arr, pats, (np.arange(len(pats)), pats))


def test_golden_fixtures_every_order():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        names = sorted(json.load(f))
    for name in names:
        with open(os.path.join(GOLDEN, name + ".text"), "rb") as f:
            s = f.read()
        arr = np.fromfile(os.path.join(GOLDEN, name + ".sa.u32le"), dtype="<u4").astype(np.uint32)
        pats = _patterns(np.random.default_rng(len(s) + 7), s, 80, max_len=3000)
        _all_orders(_u8(s), arr, pats, (np.arange(len(pats)), pats))


@pytest.mark.parametrize("gen", ["english_corpus", "uniform"])
def test_16mib_with_many_patterns(gen):
    """10^5 patterns of mixed lengths (1 .. 4096 bytes) on 16 MiB; all against the plain route, 1 500 against the model"""
    n = 16 << 20
    text = corpus.english_corpus(n, 21) if gen == "english_corpus" else corpus.uniform(n, 22)
    ix = sa.DeviceIndex(text)
    arr = ix.suffix_array()
    ix.close()
    s = text.tobytes()
    rng = np.random.default_rng(23)
    pats = _patterns(rng, s, 100_000, max_len=64)
    for q in rng.integers(8, len(pats), 3000):
        a = int(rng.integers(0, n - 4096))
        pats[int(q)] = s[a:a + int(rng.integers(65, 4097))]
    idx = rng.choice(len(pats), 1500, replace=False)
    idx[:8] = np.arange(8)                                         # the edge cases of _patterns among them
    st = _all_orders(text, arr, pats, (idx, [pats[int(q)] for q in idx]))
    assert st["compared_bytes"] <= sum(bound(len(p), n) for p in pats)


@pytest.mark.parametrize("family", ["one_byte", "fibonacci"])
def test_work_bound_on_long_patterns(family):
    """64 KiB patterns on a one-byte text of 2^20 and on a Fibonacci word: the LCP route compares at most 2 plen + 128 log2 P
    text bytes per pattern, the plain route (model figure) more than ten times that"""
    n = 1 << 20
    s = b"a" * n if family == "one_byte" else fibonacci_word(30)[:n]
    text = _u8(s)
    ix = sa.DeviceIndex(text)
    arr = ix.suffix_array()
    rng = np.random.default_rng(31)
    plen = 64 << 10
    starts = [0, n - plen] + [int(x) for x in rng.integers(0, n - plen, 6)]
    pats = [s[a:a + plen] for a in starts]
    pats.append(pats[-1][:-1] + (b"b" if pats[-1][-1:] != b"b" else b"a"))    # absent, differs in its last byte
    plain = ix.search(pats)
    ix.enable_lcp()
    got = ix.search(pats)
    st = sa.last_search_stats()
    ix.close()
    _same(got, plain, pats, family)
    assert st["route"] == 1 and st["patterns"] == len(pats)
    assert st["compared_bytes"] <= len(pats) * bound(plen, n), st
    # the plain route's figure from the model: on the one-byte text every step compares up to plen bytes (ratio ~21); on the
    # Fibonacci word a 64 KiB factor occurs a few dozen times and only the steps among those pay plen (ratio ~5)
    model_plain = plain_bytes(s, arr, pats[0])
    assert model_plain > (10 if family == "one_byte" else 4) * bound(plen, n), model_plain
    ix = sa.DeviceIndex(text, arr)
    ix.enable_lcp()
    for p in pats:                                                 # one pattern per call: the bound per pattern
        ix.search([p])
        one = sa.last_search_stats()
        assert one["compared_bytes"] <= bound(len(p), n), (family, one)
    ix.close()


N_ABOVE = (1 << 30) + 4097


def test_top_of_range_periodic(oracle):
    """a closed-form periodic text of 2^30 + 4097 bytes, array passed in: P = 2^31 and 64-bit node arithmetic; sampled patterns
    (cut from the text at phases above 2^30 too, mutated, longer than the period) agree with the model"""
    w = b"acgt"
    n = N_ABOVE
    assert log_p(n) == 31
    text = search_model.periodic_text(w, n)
    arr = search_model.periodic_sa(w, n)
    ix = sa.DeviceIndex(text, arr)
    ix.enable_lcp()
    rng = np.random.default_rng(41)
    pats = [b"", b"a", b"t", b"ta", b"tt", b"acgta", b"gtac" * 1000, b"cgt" + b"acgt" * 20000 + b"x", w * 3 + b"a"]
    for _ in range(200):
        a = int(rng.integers(0, n))
        p = bytearray(text[a:a + int(rng.integers(1, 5000))].tobytes())
        if rng.random() < 0.5:
            k = int(rng.integers(0, len(p)))
            p[k] = (p[k] + int(rng.integers(1, 256))) & 0xFF
        pats.append(bytes(p))
    pats.append(text[n - 3000:].tobytes())
    got = ix.search(pats)
    assert sa.last_search_stats()["route"] == 1
    ix.buckets()
    got_b = ix.search(pats)
    ix.close()
    bkt = oracle.bucket_table(text)
    _same(got, search_model.search_many(text, arr, pats), pats, "top of range")
    _same(got_b, search_model.search_many(text, arr, pats, bkt), pats, "top of range, buckets")
    assert int(got["lcp_start"].max()) >= 1 << 30


def test_suffix_array_enable_lcp_and_set(oracle):
    s = corpus.english(50_000, 19).tobytes()
    rng = np.random.default_rng(51)
    pats = _patterns(rng, s, 60, max_len=200)
    base = sa.SuffixArray(s)
    obj = sa.SuffixArray(s)
    obj.enable_lcp()
    for round_ in range(2):
        for p in pats:
            exp = base.contains(p), base.search_all(p), base.search_lcp(p)
            assert obj.contains(p) == exp[0], p[:40]
            assert sa.last_search_stats()["route"] == 1
            assert np.array_equal(obj.search_all(p), exp[1]), p[:40]
            assert obj.search_lcp(p) == exp[2], p[:40]
        obj.set(s)                                                 # drops the device index; the next search rebuilds it with the table
        base.enable_buckets()
        obj.enable_buckets()
