"""CPU suite (-m "not gpu"): pins the oracle against the reference's known answers, its own test
domain (reference src/tests.rs:6-17) and the committed golden fixtures."""
import json
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from conftest import KNOWN_ANSWERS, ROOT, adversarial_cases

import pd_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("text,expected", KNOWN_ANSWERS)
def test_known_answers(oracle, text, expected):
    assert oracle.naive(text).tolist() == expected
    assert oracle.sais(text).tolist() == expected
    assert oracle.check_integrity(text, np.array(expected, dtype=np.uint32)) == 1
    assert oracle.verify(text, np.array(expected, dtype=np.uint32)) == 1


def test_doctest_search_all_vector(oracle):
    """reference src/lib.rs:28-29: search_all(b"splend") == [0, 9] on b"splendid splendor"."""
    s = b"splendid splendor"
    sa = oracle.sais(s)
    hits = sorted(int(p) for p in sa if s[int(p):].startswith(b"splend"))
    assert hits == [0, 9]
    pos = [i for i, p in enumerate(sa) if int(p) in (0, 9)]
    assert pos[1] - pos[0] == 1      # one contiguous SA range


@settings(max_examples=200, deadline=None)
@given(st.binary(min_size=0, max_size=4095))
def test_conversion_correctness_domain(oracle, s):
    """reference src/tests.rs:13-17, with the oracle standing in for SuffixArray::new."""
    sa = oracle.sais(s)
    assert np.array_equal(sa, oracle.naive(s))
    assert oracle.check_integrity(s, sa) == 1
    assert oracle.verify(s, sa) == 1


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_adversarial(oracle, name):
    s = adversarial_cases()[name]
    sa = oracle.sais(s)
    assert np.array_equal(sa, oracle.naive(s))
    assert oracle.check_integrity(s, sa) == 1
    assert np.array_equal(pd_model.build(s), sa)


@settings(max_examples=120, deadline=None)
@given(st.integers(0, 2500), st.sampled_from([1, 2, 3, 4, 5, 16, 64, 200, 256]), st.integers(0, 2**32 - 1))
def test_device_algorithm_model(oracle, n, sigma, seed):
    """the numpy restatement of the GPU pipeline (packed keys, end-of-text rule, doubling)"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, sigma, n, dtype=np.uint8).tobytes()
    assert np.array_equal(pd_model.build(s), oracle.sais(s))


def test_checkers_reject_wrong_arrays(oracle):
    s = b"mississippi"
    sa = oracle.sais(s)
    bad = sa.copy(); bad[3], bad[4] = bad[4], bad[3]
    assert oracle.check_integrity(s, bad) == 0 and oracle.verify(s, bad) == 0
    assert oracle.check_integrity(s, sa[:-1]) == 0 and oracle.verify(s, sa[:-1]) == 0
    dup = sa.copy(); dup[5] = dup[6]
    assert oracle.verify(s, dup) == 0
    oob = sa.copy(); oob[2] = 99
    assert oracle.check_integrity(s, oob) == -1      # the reference panics on the slice index


def test_golden_fixtures(oracle):
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    assert len(manifest) >= 10
    for name, meta in manifest.items():
        text = open(os.path.join(GOLDEN, name + ".text"), "rb").read()
        sa = np.fromfile(os.path.join(GOLDEN, name + ".sa.u32le"), dtype="<u4")
        assert len(text) == meta["n"] and sa.size == meta["sa_len"] == len(text) + 1
        assert np.array_equal(oracle.sais(text), sa), name
        assert oracle.check_integrity(text, sa) == 1, name


def test_oracle_medium_sizes(oracle):
    from suffix_array_amd import corpus
    for text in (corpus.english(300_000, 3), corpus.dna(300_000, 4), corpus.uniform(300_000, 2),
                 corpus.dna_repeats(300_000, 5, 0.3)):
        sa = oracle.sais(text)
        assert oracle.verify(text, sa) == 1
        assert np.array_equal(pd_model.build(text.tobytes()), sa)


def test_bucket_table_restatement(oracle):
    """reference src/sa.rs:89-119: bkt[i] is the exclusive right edge of bucket i in the SA."""
    s = b"splendid splendor"
    bkt = oracle.bucket_table(s)
    sa = oracle.sais(s)
    assert bkt[0] == 1 and bkt[-1] == len(s) + 1
    c0, c1 = ord("s"), ord("p")
    idx = c0 * 257 + (c1 + 1) + 1
    rng = sa[bkt[idx - 1]:bkt[idx]]
    assert sorted(int(p) for p in rng) == [0, 9]


def test_pack_model_round_trip_and_layout():
    """numpy restatement of the packed format (reference src/packed_sa.rs); byte-level parity with the
    external bitpacking crate is unpinned, the round trip is what the reference's own test pins"""
    import pack_model
    rng = np.random.default_rng(4)
    for length in (1, 2, 3, 127, 128, 129, 255, 256, 1000, 4097):
        sa = rng.permutation(length).astype(np.uint32)
        blob = pack_model.pack(sa)
        assert np.array_equal(pack_model.unpack(blob), sa)
        bits = pack_model.sa_bits(length)
        assert len(blob) <= 16 + ((length + 127) // 128) * bits * 16
    # hand-checked block: bits = 7 for length 128; value 4 i + c of the identity sits at row i of lane c
    blob = pack_model.pack(np.arange(128, dtype=np.uint32))
    assert blob[:4] == b"SA4x" and blob[4:8] == (128).to_bytes(4, "little") and len(blob) == 16 + 7 * 16
    lane0_word0 = int.from_bytes(blob[16:20], "little")
    assert lane0_word0 & 0x7F == 0 and (lane0_word0 >> 7) & 0x7F == 4 and (lane0_word0 >> 14) & 0x7F == 8
    lane1_word0 = int.from_bytes(blob[20:24], "little")
    assert lane1_word0 & 0x7F == 1 and (lane1_word0 >> 7) & 0x7F == 5


def test_sanitized_selftest():
    """the oracle and the corpus generators under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C oracle sanitize`):
    known answers, naive sort == SA-IS == both integrity checks, the threaded verifier, every generator at ragged sizes.
    (GPU sanitizers are unavailable on this pool: the CPU side of the test infrastructure is what gets sanitized.)"""
    import shutil
    import subprocess
    if shutil.which("gcc") is None and shutil.which("cc") is None:
        pytest.skip("no C compiler")
    proc = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "sanitize"], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)
    assert proc.returncode == 0 and "selftest ok" in proc.stdout, proc.stdout[-3000:]


# ---- oracle/search_model.py: the reference's search restated (src/sa.rs:123-253), and the periodic closed form ----

def _search_texts():
    rng = np.random.default_rng(21)
    texts = [b"", b"a", b"ab", b"banana", b"mississippi", b"splendid splendor", b"a" * 300, b"ab" * 150 + b"a",
             b"\x00\xff" * 90 + b"\x00", adversarial_cases()["fib"][:700], adversarial_cases()["thue_morse"][:700]]
    texts += [rng.integers(0, sigma, int(rng.integers(1, 400)), dtype=np.uint8).tobytes() for sigma in (2, 3, 4, 256) for _ in range(3)]
    return texts


def _search_patterns(rng, s):
    pats = [b"", s, s + b"\x00", s[1:], s[-1:], s[:-1] + b"\xff", b"\x00", b"\xff", b"\xff\x00", b"zz", b"a", b"ab"]
    for _ in range(40):
        if s and rng.random() < 0.7:
            i = int(rng.integers(0, len(s))); ln = int(rng.integers(0, len(s) - i + 3))
            p = s[i:i + ln]
            if p and rng.random() < 0.4:
                p = p[:-1] + bytes([int(rng.integers(0, 256))])
        else:
            p = rng.integers(0, 4, int(rng.integers(0, 5)), dtype=np.uint8).tobytes()
        pats.append(p)
    return pats


def test_search_model_against_naive_checkers(oracle):
    """search_model without and with the bucket table against the naive checkers of the reference's own tests
    (src/tests.rs:104-132): contains, the set of search_all, and search_lcp's substring and its length"""
    import search_model as sm
    rng = np.random.default_rng(5)
    for s in _search_texts():
        arr = oracle.sais(s)
        bkt = oracle.bucket_table(s)
        assert np.array_equal(bkt, sm.bucket_table(s))
        for p in _search_patterns(rng, s):
            occ = sm.naive_search_all(s, p) if p else list(range(len(s) + 1))
            best = sm.naive_search_lcp(s, p)
            for table in (None, bkt):
                c, lo, hi, st, ln = sm.search(s, arr, p, table)
                assert c == sm.naive_contains(s, p) == (len(occ) > 0), (s, p)
                assert sorted(int(x) for x in arr[lo:hi]) == occ, (s, p)
                assert ln == len(best) and s[st:st + ln] == best, (s, p)
                assert 0 <= st <= len(s) and st + ln <= len(s)


def test_search_model_doctest_vector(oracle):
    """reference src/lib.rs:16-41: contains(splend), search_all(splend) == [0, 9], search_lcp(splash) == "spl"; and the
    empty pattern: the whole array, and the empty suffix n..n"""
    import search_model as sm
    s = b"splendid splendor"
    arr = oracle.sais(s)
    for table in (None, oracle.bucket_table(s)):
        c, lo, hi, _, _ = sm.search(s, arr, b"splend", table)
        assert c and sorted(int(x) for x in arr[lo:hi]) == [0, 9]
        _, _, _, st, ln = sm.search(s, arr, b"splash", table)
        assert s[st:st + ln] == b"spl"
        assert sm.search(s, arr, b"", table) == (True, 0, len(s) + 1, len(s), 0)
        assert sm.search(s, arr, s, table)[3:] == (0, len(s))          # Ok(i): start..s.len()
        assert sm.search(s, arr, b"dor", table)[3:] == (14, 3)


def test_search_model_with_and_without_buckets(oracle):
    """What the bucket table may change (src/sa.rs:123-160, 211-222): nothing of contains and search_all (the bucket holds
    every suffix that starts with the pattern's first bytes, and the insertion point lies inside it); search_lcp's length
    never; its START only where the pattern's bucket is empty -- there the reference answers with the first suffix of the
    top-level bucket (or s.len()..s.len()), not with a neighbour of the insertion point."""
    import search_model as sm
    from suffix_array_amd import corpus
    rng = np.random.default_rng(8)
    texts = _search_texts() + [corpus.english(20_000, 3).tobytes(), corpus.dna(5_000, 4).tobytes()]
    differ = 0
    for s in texts:
        arr = oracle.sais(s)
        bkt = sm.bucket_table(s)
        for p in _search_patterns(rng, s) + [bytes([a, b]) for a in b"\x00ae\xff" for b in b"\x00ae\xff"]:
            plain, bucketed = sm.search(s, arr, p, None), sm.search(s, arr, p, bkt)
            assert plain[:3] == bucketed[:3] and plain[4] == bucketed[4], (s, p)
            lo, hi = sm.get_bucket(s, arr, p, bkt)
            if len(p) == 0 or lo < hi:
                assert plain == bucketed, (s, p)
            elif plain[3] != bucketed[3]:
                differ += 1
                tlo, thi = sm.get_top_bucket(s, arr, p, bkt)
                assert bucketed[3] == (int(arr[tlo]) if thi > tlo else len(s))
    assert differ > 0                   # (the two answers really do differ somewhere: the comparison has teeth)


def test_search_model_reads_a_large_text_in_place():
    """a numpy text is read a pattern's length at a time, never copied: a 256 MiB text of one byte searched in milliseconds"""
    import time
    import search_model as sm
    n = 256 << 20
    s = np.full(n, 7, dtype=np.uint8)
    arr = np.arange(n, -1, -1, dtype=np.uint32)          # (the closed form of a one-byte text)
    t0 = time.perf_counter()
    assert sm.search(s, arr, b"\x07" * 100, None) == (True, 100, n + 1, n - 100, 100)       # Ok(i): the suffix of length 100
    assert sm.search(s, arr, b"\x07" * 5 + b"\x08", None) == (False, n + 1, n + 1, 0, 5)     # above every suffix: sa[len - 1]
    assert time.perf_counter() - t0 < 5.0


@pytest.mark.parametrize("w", [b"abc", b"\xff\x61\x00\x63", b"x", b"cab", b"\x00\x05\xff\x80\x01"])
def test_periodic_closed_form(oracle, w):
    """the suffix array of a prefix of w w w ... (w of distinct bytes) is [n], then each phase by its byte, positions
    descending -- against SA-IS at every length up to 600 and at ragged lengths up to 4096; the sliced comparator agrees,
    and finds a swap"""
    import search_model as sm
    for n in list(range(0, 600)) + [1023, 1024, 1025, 4095, 4096]:
        s = sm.periodic_text(w, n)
        exp = oracle.sais(s)
        assert np.array_equal(sm.periodic_sa(w, n), exp), n
        assert sm.periodic_mismatch(exp, w, n, chunk=7) is None, n
        if n >= 3:
            bad = exp.copy(); bad[n - 1], bad[n] = bad[n], bad[n - 1]
            assert sm.periodic_mismatch(bad, w, n, chunk=5) == n - 1
