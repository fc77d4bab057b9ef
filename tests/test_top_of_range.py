"""GPU suite, top of the size range (-m gpu): texts between 2^30 and MAX_LENGTH = 2^31 - 1 through the host-pointer ABI.

Above 2^30 the indices take 31 bits: the first pass of the 32-bit stage has room for ONE key bit in a value word
(val_extra = 32 - g_bits, host/pipeline.hpp; carried through the passes by host/sort.hpp), the refinement rounds carry ranks and suffix indices >= 2^30, and the packed
format is 31 bits wide.  Every build names the route it is meant to cover and asserts it through last_stats(), so a later
tuning change cannot quietly turn one case into a copy of another.  Arrays are checked against a closed form where one
exists (periodic texts, oracle/search_model.py), otherwise with the oracle's linear-time verifier, the GPU integrity check and
sampled neighbour comparisons.

At most two large texts are alive at once: the module-scoped fixture at the end holds one, and its tests come last.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus

import pack_model
import search_model

pytestmark = pytest.mark.gpu

N_ABOVE = (1 << 30) + 4097          # odd, just above 2^30: g_bits = 31


def _build(text):
    arr = np.empty(text.size + 1, dtype=np.uint32)
    sa.saca(text, arr)
    return arr, sa.last_stats()


def _sampled_neighbours_ordered(text, arr, seed, samples=3000, width=256, lo=1):
    rng = np.random.default_rng(seed)
    n = text.size
    for i in rng.integers(lo, n, samples):
        a, b = int(arr[i]), int(arr[i + 1])
        x, y = text[a:a + width].tobytes(), text[b:b + width].tobytes()
        assert x < y or (x == y and len(x) == width), (i, a, b)


def _check_generated(oracle, text, arr):
    assert arr[0] == text.size
    assert oracle.verify_mt(text, arr, 16) == 1
    assert sa.check_integrity(text, arr) is True
    _sampled_neighbours_ordered(text, arr, 11)
    _sampled_neighbours_ordered(text, arr, 12, samples=1000, lo=1 << 30)       # slots holding ranks >= 2^30


def _check_periodic(text, arr, w):
    n = text.size
    assert search_model.periodic_mismatch(arr, w, n) is None
    assert sa.check_integrity(text, arr) is True
    _sampled_neighbours_ordered(text, arr, 13, samples=500)


@pytest.fixture
def _release():
    yield
    sa.lib().sa_amd_release_cache()


# ---- closed forms: full equality -------------------------------------------------------------------------------------

def test_max_length_one_byte_general_path_and_closed_form(monkeypatch, _release):
    """MAX_LENGTH copies of one byte.  Route 1, general path (the suite keeps SA_AMD_NO_UNARY_SHORTCUT=1): one group of
    2^31 - 1 members through every doubling round, ranks and indices up to 2^31 - 1.  Route 2, the knob removed: the closed
    form k_fill_descending (no sort, no rounds).  Both equal to SA[i] = n - i."""
    n = sa.MAX_LENGTH
    text = np.full(n, 0x61, dtype=np.uint8)
    arr, st = _build(text)
    assert st["sigma"] == 1 and st["rounds"] > 0 and st["sort_passes"] > 0, st
    _check_periodic(text, arr, b"a")
    arr.fill(0)
    monkeypatch.delenv("SA_AMD_NO_UNARY_SHORTCUT", raising=False)
    sa.saca(text, arr)
    st = sa.last_stats()
    assert st["sigma"] == 1 and st["rounds"] == 0 and st["sort_passes"] == 0, st
    assert search_model.periodic_mismatch(arr, b"a", n) is None


def test_max_length_abc(_release):
    """MAX_LENGTH bytes of abcabc...: three giant groups (one per phase) refined by doubling up to 2^31 - 1"""
    n = sa.MAX_LENGTH
    text = search_model.periodic_text(b"abc", n)
    arr, st = _build(text)
    assert st["sigma"] == 3 and st["rounds"] > 0, st
    _check_periodic(text, arr, b"abc")


def test_period_five_with_zero_and_ff_above_2_30(_release):
    """a period-5 word holding 0x00 and 0xff, odd length just above 2^30: the extreme byte values as phase heads of five giant
    groups, indices of 31 bits"""
    w = b"\x80\x00\xff\x01\x7f"
    text = search_model.periodic_text(w, N_ABOVE)
    arr, st = _build(text)
    assert st["sigma"] == 5 and st["rounds"] > 0, st
    _check_periodic(text, arr, w)


# ---- generated texts just above 2^30 -----------------------------------------------------------------------------------

def test_dna_above_2_30_packed_keys_with_one_value_bit(oracle, _release):
    """DNA (sigma 4, 2-bit codes) of 2^30 + 4097 bytes: the 32-bit first stage reading the bit-packed text as its key stream
    (packed_keys), with ONE key bit below the 32 in the top of each value word (g_bits = 31)"""
    text = corpus.dna(N_ABOVE, 41)
    arr, st = _build(text)
    assert st["sigma"] == 4 and st["bits_per_symbol"] == 2 and st["top32_first"] == 1, st
    _check_generated(oracle, text, arr)


def test_dna_repeats_above_2_30_doubling_rounds(oracle, _release):
    """DNA with 20 % planted repeats (1-100 KiB, 1 % mutations), 2^30 + 4097 bytes: long ties resolved by at least two
    refinement rounds over ranks and indices >= 2^30"""
    text = corpus.dna_repeats(N_ABOVE, 42, 0.2)
    arr, st = _build(text)
    assert st["sigma"] == 4 and st["rounds"] >= 2, st
    _check_generated(oracle, text, arr)


def test_english_corpus_above_2_30_text_rounds_then_doubling(oracle, monkeypatch, _release):
    """English-like corpus with copied passages, 2^30 + 4097 bytes: text-keyed rounds (secondary key read from the text) and
    then rank doubling for the copies they cannot finish.  The repeat probe would send a corpus this repetitive straight to
    doubling; SA_AMD_NO_REPEAT_PROBE (result-neutral) pins the route with both kinds of round."""
    monkeypatch.setenv("SA_AMD_NO_REPEAT_PROBE", "1")
    text = corpus.english_corpus(N_ABOVE, 43)
    arr, st = _build(text)
    assert st["text_rounds"] >= 1 and st["rounds"] > st["text_rounds"], st
    _check_generated(oracle, text, arr)


def _planted(n, seed, copies):
    """uniform random bytes with `copies` copied segments of 20-3000 bytes: few tied suffixes after the initial sort"""
    rng = np.random.default_rng(seed)
    s = corpus.uniform(n, seed)
    for _ in range(copies):
        ln = int(rng.integers(20, 3000))
        src = int(rng.integers(0, n - ln)); dst = int(rng.integers(0, n - ln))
        s[dst:dst + ln] = s[src:src + ln]
    for dst in (n - 2000, (1 << 30) + 5):                         # copies ending at the text's end and sitting above 2^30
        src = int(rng.integers(0, 1 << 29))
        s[dst:dst + 1500] = s[src:src + 1500]
    return s


def test_planted_bytes_above_2_30_text_keys_and_sparse_rounds(oracle, _release):
    """random bytes with planted copies, 2^30 + 4097 bytes: the 32-bit first stage reading its keys from the text (text_keys,
    sigma 256, one value bit) and the sparse refinement mode (ranks by binary search in the sorted keys) over suffixes >= 2^30"""
    text = _planted(N_ABOVE, 44, 300)
    arr, st = _build(text)
    assert st["sigma"] == 256 and st["bits_per_symbol"] == 8 and st["top32_first"] == 1, st
    assert st["sparse_mode"] == 1 and st["rounds"] >= 1 and 0 < st["unresolved_after_initial"] <= text.size // 64, st
    _check_generated(oracle, text, arr)


# ---- one text kept for the device-resident extras ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(oracle):
    """dna_repeats of 2^30 + 4097 bytes and its array (host-pointer build, verified).  The conftest's autouse fixture is
    function-scoped and runs after this one, so the unary knob is set here for the build"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SA_AMD_NO_UNARY_SHORTCUT", "1")
        text = corpus.dna_repeats(N_ABOVE, 45, 0.2)
        arr, st = _build(text)
        assert st["rounds"] >= 2, st
    assert arr[0] == text.size and oracle.verify_mt(text, arr, 16) == 1
    yield text, arr
    sa.lib().sa_amd_release_cache()


def _top_patterns(rng, s, n):
    """patterns taken at positions >= 2^30 and at the end of the text, some mutated, some of several 64-byte chunks"""
    end = [_piece(s, n - k, k) for k in (1, 5, 300, 4096)]                 # suffixes: Ok(i), start..s.len()
    pats = [b"", b"A", b"T", b"\x00", b"\xff", b"AC\xff", b"N"] + end + [e + b"A" for e in end] + [e[:-1] + b"\x00" for e in end]
    for ln in (1, 2, 3, 8, 16, 31, 63, 64, 65, 128, 129, 4096):
        for _ in range(20):
            i = int(rng.integers(1 << 30, n - ln))
            p = _piece(s, i, ln)
            if rng.random() < 0.4:
                k = int(rng.integers(0, ln))
                p = p[:k] + bytes([(p[k] + 1 + int(rng.integers(0, 254))) & 255]) + p[k + 1:]
            pats.append(p)
    for _ in range(40):
        i = int(rng.integers(0, 1 << 30))
        pats.append(_piece(s, i, int(rng.integers(1, 40))))
    return pats


def _piece(s, i, ln):
    return s[i:i + ln].tobytes()


def test_device_index_at_the_top(oracle, big):
    """DeviceIndex on the 2^30 + 4097-byte text, array built on the device: it equals the host build, passes the integrity
    check, its bucket table (binary search over the array, k_bucket_table) equals the oracle's, and a few hundred searches
    equal the reference's (oracle/search_model.py) before and after the bucket table"""
    text, arr = big
    n = text.size
    ix = sa.DeviceIndex(text)
    assert np.array_equal(ix.suffix_array(), arr)
    assert ix.check_integrity()
    rng = np.random.default_rng(46)
    pats = _top_patterns(rng, text, n)
    got = ix.search(pats)
    exp = search_model.search_many(text, arr, pats)
    for k in exp:
        assert np.array_equal(got[k], exp[k]), (k, [p[:40] for p, g, e in zip(pats, got[k], exp[k]) if g != e][:3])
    assert int(got["lcp_start"].max()) >= 1 << 30                 # answers above 2^30 really are there
    bkt = oracle.bucket_table(text)
    assert np.array_equal(ix.buckets(), bkt)
    got = ix.search(pats)
    exp = search_model.search_many(text, arr, pats, bkt)
    for k in exp:
        assert np.array_equal(got[k], exp[k]), (k, [p[:40] for p, g, e in zip(pats, got[k], exp[k]) if g != e][:3])
    ix.close()


@contextlib.contextmanager
def _mutated(arr, idx, vals):
    """arr[idx] = vals for the block, then the old entries back (no copy of the 4 GiB array)"""
    old = arr[idx].copy()
    arr[idx] = vals
    try:
        yield arr
    finally:
        arr[idx] = old


def test_integrity_check_at_the_top(big):
    """the GPU integrity check (reference src/sa.rs:72-84) on the large array, host-pointer form and both work-block forms of
    sa_amd_check_integrity_device: the good array, adjacent swaps above 2^30, a duplicate, an entry of n + 7 (the reference
    panics: IndexError / -6), a rotated window"""
    text, arr = big
    n = text.size
    rng = np.random.default_rng(47)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    L = sa.lib()
    big_wb, small_wb = int(L.sa_amd_check_integrity_work_bytes(n)), 4 * (n + 1) + 256
    dt, ds, dw = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dt), n + 64) == 0 and hip.hipMalloc(ctypes.byref(ds), 4 * (n + 1) + 64) == 0
    assert hip.hipMalloc(ctypes.byref(dw), big_wb + 512) == 0
    work = (dw.value + 255) & ~255
    try:
        assert hip.hipMemcpy(dt.value, text.ctypes.data, n, 1) == 0

        def forms(a):
            try:
                host = sa.check_integrity(text, a)
            except IndexError:
                host = -6
            assert hip.hipMemcpy(ds.value, a.ctypes.data, 4 * (n + 1), 1) == 0
            return (int(host), L.sa_amd_check_integrity_device(dt.value, n, ds.value, work, big_wb, None),
                    L.sa_amd_check_integrity_device(dt.value, n, ds.value, work, small_wb, None))

        assert forms(arr) == (1, 1, 1)
        for i in [n - 1] + rng.integers(1 << 30, n, 2).tolist():
            i = int(i)
            with _mutated(arr, [i, i + 1], [arr[i + 1], arr[i]]):
                assert forms(arr) == (0, 0, 0), i
        # the slots where the streaming check takes separate paths: first-byte boundaries (skipped by the slot-order pass,
        # proved by k_ci_first_bytes), the first lane of a wave and of a workgroup (no shuffle: SA[i - 1] fetched) above
        # 2^30, and suffix n - 1 (its next suffix is the empty one)
        counts = np.bincount(text, minlength=256)
        starts = 1 + np.cumsum(counts) - counts
        slots = [int(s) - 1 for c, s in enumerate(starts) if counts[c] and s > 1]
        lane0 = ((1 << 30) + 64) & ~63
        last0 = (n - 2) & ~63
        slots += [lane0, lane0 + 1, last0, last0 + 1, (1 << 30) + 2048]
        r = int(np.flatnonzero(arr == n - 1)[0])
        slots += [r - 1, r]
        for i in slots:
            assert 0 <= i < n, i
            with _mutated(arr, [i, i + 1], [arr[i + 1], arr[i]]):
                assert forms(arr) == (0, 0, 0), i
        j = int(rng.integers(1 << 30, n))
        with _mutated(arr, [j], [arr[j + 1]]):                             # a value twice, another one missing
            assert forms(arr) == (0, 0, 0)
        with _mutated(arr, [j], [n + 7]):
            assert forms(arr) == (-6, -6, -6)
        w = slice(j - 100_000, j + 100_000)
        with _mutated(arr, w, np.roll(arr[w], 1)):                         # a permutation, in order almost everywhere
            assert forms(arr) == (0, 0, 0)
        assert forms(arr) == (1, 1, 1)                                     # (restored)
    finally:
        for p in (dt, ds, dw):
            hip.hipFree(p)


def test_packed_format_at_31_bits(big):
    """the packed format of the (2^30 + 4098)-entry array: 31 bits per entry (src/packed_sa.rs:127-129), header fields, byte
    equality with pack_model on the first and last full blocks, ~2 000 random full blocks and the trimmed last partial
    block (block b at 16 + b * bits * 16), and the round trip"""
    _, arr = big
    length = arr.size
    bits = pack_model.sa_bits(length)
    assert bits == 31 and length % 128 != 0
    blob = sa.pack(arr)
    full = length // 128
    assert blob[:4] == b"SA4x" and int.from_bytes(blob[4:8], "little") == length
    assert int.from_bytes(blob[8:16], "little") == len(blob) - 16
    tail = pack_model.block_bytes(arr, full)
    assert len(blob) == 16 + full * bits * 16 + len(tail) and blob[16 + full * bits * 16:] == tail
    rng = np.random.default_rng(48)
    for b in [0, full - 1] + rng.integers(0, full, 2000).tolist() + rng.integers((1 << 30) // 128, full, 200).tolist():
        at = 16 + int(b) * bits * 16
        assert blob[at:at + bits * 16] == pack_model.block_bytes(arr, int(b)), b
    back = sa.unpack(blob)
    del blob
    assert np.array_equal(back, arr)
