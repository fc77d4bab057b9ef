"""CPU suite for scoring a text under the infinity-gram model: the definitions of include/suffix_array_amd.h (S, LO, HI, AT_END,
NLO, NHI per query position) restated over infgram_definition / next_bytes_definition of tests/test_ngram_abi.py and checked
against literal brute force on the raw bytes; pure-Python models of gallop + bisection, of the long decision and of the work
bounds of DESIGN.md section 22; the exports, the Python surface and the argument checks that answer without a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases
from test_docs_abi import _u8, range_definition
from test_ngram_abi import EXAMPLE_SA, EXAMPLE_TEXT, brute_starts, ceil_log2, infgram_definition

EXPORTS = ("sa_amd_index_infgram_score", "sa_amd_index_infgram_score_device", "sa_amd_score_work_bytes", "sa_amd_last_score_stats",
           "sa_amd_score_set_group_cap")
STATS_FIELDS = ("positions", "documents", "group_searches", "long_searches", "next_lookups", "compared_bytes", "long_positions",
                "zero_positions", "group_cap", "readbacks")
NAMES = ("s", "lo", "hi", "at_end", "nlo", "nhi")
TILE = 256
GROUP_CHUNK = 32                                                      # bytes a group of 8 lanes compares a round, charged whole
WAVE_CHUNK = 64                                                       # the long path's wave compare


# ---------------------------------------------------------------- the definitions ----

def doc_starts(m, q_off):
    """per position the start of its document (the largest offset that is not above it)"""
    if q_off is None:
        return np.zeros(m, dtype=np.int64)
    off = np.asarray(q_off, dtype=np.int64)
    return off[np.searchsorted(off, np.arange(m), "right") - 1]


def score_definition(text, arr, query, q_off, min_count, max_len):
    """-> dict of int64 arrays s / lo / hi / at_end / nlo / nhi over the positions of the query: infgram_definition of the prompt
    Q[start .. j) gives the first four, its next[] gives NLO = LO + AT_END + sum(next[b'] for b' < Q[j]) and NHI = NLO + next[Q[j]]"""
    tb, qb = bytes(text), bytes(query)
    m = len(qb)
    out = {k: np.zeros(m, dtype=np.int64) for k in NAMES}
    start = doc_starts(m, q_off)
    for j in range(m):
        s, lo, hi, ae, nxt, _ = infgram_definition(tb, arr, qb[int(start[j]):j], min_count, max_len)
        nlo = lo + ae + int(nxt[:qb[j]].sum())
        for k, v in zip(NAMES, (s, lo, hi, ae, nlo, nlo + int(nxt[qb[j]]))):
            out[k][j] = v
    return out


def brute_score(tb, qb, q_off, min_count, max_len):
    """the same from the raw bytes alone: occurrences counted by slicing, every length tried longest first, a slot number as the
    count of the suffixes (the empty one included) that sort below the string"""
    n, m = len(tb), len(qb)
    out = {k: np.zeros(m, dtype=np.int64) for k in NAMES}
    start = doc_starts(m, q_off)

    def below(x):
        return sum(1 for i in range(n + 1) if tb[i:i + len(x)] < x)
    for j in range(m):
        cap = min(j - int(start[j]), max_len)
        s = next((k for k in range(cap, 0, -1) if len(brute_starts(tb, qb[j - k:j], min_count)) >= min_count), 0)
        ctx = qb[j - s:j]
        occ = len(brute_starts(tb, ctx))
        full = ctx + qb[j:j + 1]
        for k, v in zip(NAMES, (s, below(ctx), below(ctx) + occ, int(tb.endswith(ctx)), below(full), below(full) + len(brute_starts(tb, full)))):
            out[k][j] = v
    return out


# ---------------------------------------------------------------- the routes' models ----

def effective_group_cap(group_cap, max_len):
    """ge of kernels/score.hpp: min(group cap, max_len, 4096); a negative cap is the default"""
    return min(sa.SCORE_GROUP_CAP_DEFAULT if group_cap < 0 else group_cap, max_len, sa.SCORE_MAX_CONTEXT)


def gallop_model(ok, cap, ge=1 << 30):
    """the probe sequence of kernels/score.hpp for one position.  ok(s): the suffix of s bytes occurs often enough (monotone).
    The group path gallops s = 1, 2, 4, ... clamped to min(cap, ge) until a probe fails or the clamp holds; with ge good and
    cap > ge the position is long and the gallop goes on from the next power of two, clamped to cap; a bisection between the
    last good and the first bad length ends either.  -> (S, lengths probed on the group path, on the long path, is_long)"""
    good, bad, step, limit = 0, cap + 1, 1, min(cap, ge)
    group, long_ = [], []

    def probe(s, into):
        nonlocal good, bad
        into.append(s)
        if ok(s):
            good = s
        else:
            bad = s
    while good < limit and bad > cap:
        probe(min(step, limit), group)
        step <<= 1
    is_long = bad > cap and cap > ge
    if is_long:
        step = 1
        while step <= good:
            step <<= 1
        while good < cap and bad > cap:
            probe(min(step, cap), long_)
            step <<= 1
    while bad - good > 1:
        probe((good + bad) // 2, long_ if is_long else group)
    return good, group, long_, is_long


def gallop_bound(s):
    """range searches of one position with answer s, whatever the caps"""
    return 2 * ceil_log2(s + 2) + 2


def long_decision(cap, s, ge):
    """a position goes to the long list iff its document allows more than ge bytes of context and ge bytes are good -- the
    count never grows with the length, so that is S >= ge"""
    return cap > ge and s >= ge


def predicted_long_positions(m, q_off, S, max_len, group_cap):
    """long_positions of the statistics for a group cap, from the uncapped definition's S"""
    ge = effective_group_cap(group_cap, max_len)
    start = doc_starts(m, q_off)
    return sum(1 for j in range(m) if long_decision(min(j - int(start[j]), max_len), int(S[j]), ge))


def search_steps_bound(n):
    """text compares of one range search: two binary searches over at most n + 1 slots, or two descents of ceil(log2(n + 2))
    levels over the LCP table"""
    return 2 * (ceil_log2(n + 2) + 1)


def compared_bytes_bound(n, group_lengths, long_lengths):
    """a compare never looks past the pattern's s bytes and chunks are charged whole"""
    steps = search_steps_bound(n)
    return steps * (sum(GROUP_CHUNK * -(-s // GROUP_CHUNK) for s in group_lengths) + sum(WAVE_CHUNK * -(-s // WAVE_CHUNK) for s in long_lengths))


def position_models(text, arr, query, q_off, min_count, max_len, group_cap):
    """gallop_model of every position over range_definition -> list of (S, group lengths, long lengths, is_long)"""
    tb, qb = bytes(text), bytes(query)
    start = doc_starts(len(qb), q_off)
    ge = effective_group_cap(group_cap, max_len)
    out = []
    for j in range(len(qb)):
        def ok(s):
            lo, hi = range_definition(tb, arr, qb[j - s:j])
            return hi - lo >= min_count
        out.append(gallop_model(ok, min(j - int(start[j]), max_len), ge))
    return out


# ---------------------------------------------------------------- the cases ----

def queries_of(tb, rng):
    """(query, q_off) pairs: pieces of the text with substituted bytes, a byte the text lacks, the text's last bytes at a
    document's end, empty documents at the front, in the middle and at the end"""
    n = len(tb)
    absent = bytes([next((c for c in range(255, -1, -1) if c not in set(tb)), 0)])
    parts = []
    for _ in range(3):
        if n:
            a = int(rng.integers(0, n))
            piece = bytearray(tb[a:a + int(rng.integers(1, 24))])
            parts.append(bytes(piece))
            piece[int(rng.integers(0, len(piece)))] ^= 0x55
            parts.append(bytes(piece))
    parts += [absent + tb[:3], tb[-9:] + absent]                           # (the last context is the text's tail: at_end)
    qb = b"".join(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    holes = np.concatenate([[0, 0], off[:3], off[2:], [len(qb)]]).astype(np.int64)           # empty documents: front, middle, end
    return [(qb, None), (qb, off), (qb, holes), (tb[-5:] + tb[:30], np.array([0, min(5, n), min(5, n) + len(tb[:30])], dtype=np.int64))]


def _check_text(tb, oracle, rng):
    n = len(tb)
    arr = oracle.sais(_u8(tb))
    for qb, q_off in queries_of(tb, rng):
        for min_count, max_len in ((1, 4096), (2, 4096), (1, 1), (1, 3), (n + 2, 7)):
            d = score_definition(tb, arr, qb, q_off, min_count, max_len)
            b = brute_score(tb, qb, q_off, min_count, max_len)
            for k in NAMES:
                assert np.array_equal(d[k], b[k]), (k, qb[:16], min_count, max_len)
            start = doc_starts(len(qb), q_off)
            assert np.all(d["s"] <= np.minimum(np.arange(len(qb)) - start, max_len))
            assert np.all((d["lo"] + d["at_end"] <= d["nlo"]) & (d["nlo"] <= d["nhi"]) & (d["nhi"] <= d["hi"]))
            if min_count == n + 2:
                assert not d["s"].any() and np.all(d["hi"] - d["lo"] == n + 1) and np.all(d["at_end"] == 1)
            for j in np.flatnonzero(d["nhi"] > d["nlo"]):                                # the sub-range is the range of context + byte
                assert range_definition(tb, arr, qb[j - int(d["s"][j]):j + 1]) == (int(d["nlo"][j]), int(d["nhi"][j]))
            for ge in (0, 1, 3, 4, 64, 1 << 30):
                models = position_models(tb, arr, qb, q_off, min_count, max_len, ge)
                assert [mo[0] for mo in models] == d["s"].tolist(), (ge, min_count, max_len)
                for (s, group, long_, is_long), j in zip(models, range(len(qb))):
                    cap = min(j - int(start[j]), max_len)
                    assert len(group) + len(long_) <= gallop_bound(s), (s, group, long_, ge)
                    assert is_long == long_decision(cap, s, effective_group_cap(ge, max_len))
                    assert all(x <= effective_group_cap(ge, max_len) for x in group) and (is_long or not long_)
                assert sum(mo[3] for mo in models) == predicted_long_positions(len(qb), q_off, d["s"], max_len, ge)


# ---------------------------------------------------------------- the tests ----

def test_the_header_example(oracle):
    arr = oracle.sais(_u8(EXAMPLE_TEXT))
    assert arr.tolist() == EXAMPLE_SA
    rows = {0: (0, 0, 12, 1, 12, 12), 1: (0, 0, 12, 1, 8, 9), 2: (1, 8, 9, 0, 8, 9), 3: (2, 8, 9, 0, 8, 8), 4: (2, 2, 4, 0, 2, 4), 5: (3, 2, 4, 0, 2, 4)}
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    for fn in (score_definition, brute_score):
        d = fn(EXAMPLE_TEXT, arr, b"xcabra", None, 1, 4) if fn is score_definition else fn(EXAMPLE_TEXT, b"xcabra", None, 1, 4)
        for j, row in rows.items():
            assert tuple(int(d[k][j]) for k in NAMES) == row, (fn.__name__, j)
    for j, (s, lo, hi, ae, nlo, nhi) in rows.items():
        line = f"{j}  {chr(b'xcabra'[j])}     {s}  [{lo}, {hi})".ljust(22) + f"{ae}       [{nlo}, {nhi})"
        assert line in header, line
    assert int(score_definition(EXAMPLE_TEXT, arr, b"xcabra", None, 3, 4)["s"][5]) == 0
    assert "With min_count = 3, position 5 has S = 0" in header
    assert "#define SA_AMD_SCORE_MAX_CONTEXT 4096" in header
    _check_text(EXAMPLE_TEXT, oracle, np.random.default_rng(31))


@pytest.mark.parametrize("name", sorted(k for k, v in adversarial_cases().items() if len(v) <= 1400))
def test_definition_against_brute_force_adversarial(oracle, name):
    tb = adversarial_cases()[name]
    _check_text(tb, oracle, np.random.default_rng(len(tb) + 3))


@pytest.mark.parametrize("sigma", [1, 2, 4, 256])
def test_definition_against_brute_force_random(oracle, sigma):
    rng = np.random.default_rng(sigma + 40)
    for n in (0, 1, 2, 7, 64, 65, 300):
        _check_text(rng.integers(0, sigma, n).astype(np.uint8).tobytes(), oracle, rng)


def test_gallop_model_on_every_answer():
    """whatever the answer S in 0 .. cap and the group cap: the model finds S, within 2 ceil(log2(S + 2)) + 2 probes, the group
    path never probes more than ge bytes, and the long decision is S >= ge with room for more"""
    for cap in list(range(0, 40)) + [63, 64, 65, 255, 256, 257, 4095, 4096]:
        answers = range(cap + 1) if cap <= 70 else sorted({0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, cap - 1, cap})
        for want in answers:
            for ge in (0, 1, 2, 3, 4, 5, 16, 63, 64, 65, 4096):
                s, group, long_, is_long = gallop_model(lambda x: x <= want, cap, ge)
                assert s == want and len(group) + len(long_) <= gallop_bound(want), (cap, want, ge, group, long_)
                assert all(1 <= x <= min(cap, ge) for x in group) and all(ge < x <= cap for x in long_)
                assert is_long == long_decision(cap, want, ge) and (is_long or not long_)
            if cap:                                                    # a power-of-two group cap never changes the probe sequence
                seqs = {tuple(g + l) for g, l in (gallop_model(lambda x: x <= want, cap, ge)[1:3] for ge in (0, 1, 4, 64, 4096))}
                assert len(seqs) == 1
    assert [gallop_bound(s) for s in (0, 1, 2, 6, 7, 4096)] == [4, 6, 6, 8, 10, 28]
    assert gallop_model(lambda x: x <= 5, 4096)[1] == [1, 2, 4, 8, 6, 5]                 # (the bisection's cost at cap 4096 would be 13)


def test_bounds_of_the_work_model():
    assert (search_steps_bound(0), search_steps_bound(11), search_steps_bound((1 << 20))) == (4, 10, 44)
    assert compared_bytes_bound(11, [1, 32, 33], [64, 65]) == 10 * (32 + 32 + 64 + 64 + 128)
    assert [effective_group_cap(c, ml) for c, ml in ((-1, 4096), (-1, 5), (0, 4096), (1 << 20, 4096), (1 << 20, 100), (4, 64))] == [64, 5, 0, 4096, 100, 4]


# ---------------------------------------------------------------- the surface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    body = header[header.index("typedef struct sa_amd_score_stats"):header.index("} sa_amd_score_stats;")]
    declared = re.findall(r"^\s+int(64|32)_t\s+(\w+);", body, re.M)
    assert [name for _, name in declared] == list(STATS_FIELDS) == [name for name, _ in sa.ScoreStats._fields_]
    for (bits, name), (_, ctype) in zip(declared, sa.ScoreStats._fields_):
        assert ctypes.sizeof(ctype) * 8 == int(bits), name
    assert ctypes.sizeof(sa.ScoreStats) == 8 * 8 + 2 * 4
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "score.hpp")) as f:
        kernels = f.read()
    for name, value in (("SCORE_CAP_DEFAULT", sa.SCORE_GROUP_CAP_DEFAULT), ("SCORE_STAGE_MAX", sa.SCORE_MAX_CONTEXT), ("SCORE_TILE", sa.SCORE_TILE)):
        m = re.search(r"constexpr int " + name + r" = ([^;]+);", kernels)
        assert m and int(m.group(1)) == value, name
    assert (sa.SCORE_GROUP_CAP_DEFAULT, sa.SCORE_MAX_CONTEXT, sa.SCORE_TILE) == (64, 4096, TILE)
    with open(os.path.join(ROOT, "include", "suffix_array_amd.hpp")) as f:
        assert "infgram_score(" in f.read()


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        assert params(cls.infgram_score) == ["self", "query", "min_count", "max_len", "doc_offsets"]
        sig = inspect.signature(cls.infgram_score).parameters
        assert [sig[k].default for k in ("min_count", "max_len", "doc_offsets")] == [1, sa.SCORE_MAX_CONTEXT, None]
    assert params(sa.score_set_group_cap) == ["nbytes"] and params(sa.last_score_stats) == []
    for name in ("ScoreStats", "ScoreResult", "last_score_stats", "score_set_group_cap", "score_work_bytes", "infgram_score_device_ptr",
                 "SCORE_MAX_CONTEXT", "SCORE_GROUP_CAP_DEFAULT"):
        assert name in sa.__all__ and hasattr(sa, name), name
    assert set(sa.last_score_stats()) == set(STATS_FIELDS) | {"range_searches"}


def test_result_object_on_the_header_example(oracle):
    """log2_prob and doc_bits are numpy on the host: the example's rows give p = 0, 1/11, 1, 0, 1, 1"""
    arr = oracle.sais(_u8(EXAMPLE_TEXT))
    d = score_definition(EXAMPLE_TEXT, arr, b"xcabra", None, 1, 4)
    r = sa.ScoreResult(*(d[k].astype(np.uint8 if k == "at_end" else np.uint32) for k in NAMES))
    assert len(r) == 6 and [a.tolist() for a in r] == [d[k].tolist() for k in NAMES]
    lp = r.log2_prob()
    assert lp.dtype == np.float64 and np.isneginf(lp[[0, 3]]).all() and lp[[2, 4, 5]].tolist() == [0.0, 0.0, 0.0]
    assert lp[1] == pytest.approx(-np.log2(11.0), abs=1e-12)
    bits, zeros = r.doc_bits()
    assert bits.tolist() == [pytest.approx(np.log2(11.0))] and zeros.tolist() == [1 + 1]
    bits, zeros = r.doc_bits([0, 0, 2, 6, 6])
    assert bits.tolist() == [0.0, pytest.approx(np.log2(11.0)), 0.0, 0.0] and zeros.tolist() == [0, 1, 1, 0]
    # a denominator of 0: the context occurs only as the text's last bytes
    z = sa.ScoreResult(*(np.array(v, dtype=np.uint32) for v in ([3], [5], [6], [1], [6], [6])))
    assert np.isneginf(z.log2_prob()).all() and z.doc_bits()[1].tolist() == [1]
    e = sa.ScoreResult(*(np.zeros(0, dtype=np.uint32) for _ in range(6)))
    assert e.log2_prob().size == 0 and e.doc_bits()[0].tolist() == [0.0] and e.doc_bits([0, 0, 0])[1].tolist() == [0, 0]


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    fake = ctypes.c_void_p(p)                                         # never dereferenced: every check below fails before the index is used
    good = np.array([0, 2, 4], dtype=np.int64)
    g = good.ctypes.data

    def host(ix, q, m, off, ndocs, min_count, max_len):
        return L.sa_amd_index_infgram_score(ix, q, m, off, ndocs, min_count, max_len, p, p, p, p, p, p)

    def dev(ix, q, m, off, ndocs, min_count, max_len):
        return L.sa_amd_index_infgram_score_device(ix, q, m, off, ndocs, min_count, max_len, p, p, p, p, p, p, p, 1 << 20, None)
    for call in (host, dev):
        assert call(None, p, 4, g, 2, 1, 8) == -1                                                # NULL index
        assert call(fake, p, -1, None, 0, 1, 8) == -1                                            # negative m
        assert call(fake, None, 4, None, 0, 1, 8) == -1                                          # no query
        assert call(fake, p, 4, g, -1, 1, 8) == -1                                               # negative ndocs
        for min_count in (0, -1, -2**31):
            assert call(fake, p, 4, g, 2, min_count, 8) == -1
        for max_len in (0, -1, 4097, 2**31 - 1):
            assert call(fake, p, 4, g, 2, 1, max_len) == -1
        for off in ([1, 2, 4], [0, 3, 2], [0, 2, 5], [0, 2, 3], [-1, 2, 4], [0, 5, 4]):       # malformed q_off
            a = np.array(off, dtype=np.int64)
            assert call(fake, p, 4, a.ctypes.data, 2, 1, 8) == -1, off
    assert np.all(buf == 0x77777777)
    assert L.sa_amd_score_work_bytes(-1, 1) == -1 and L.sa_amd_score_work_bytes(5, -1) == -1
    assert L.sa_amd_score_work_bytes(0, 0) > 0 and L.sa_amd_score_work_bytes(1 << 20, 3) >= 12 * (1 << 20)
    L.sa_amd_last_score_stats(None)
    with pytest.raises(sa.SuffixArrayError):                                                     # refused before the index is touched
        sa.DeviceIndex.infgram_score(None, b"abc", min_count=0)
    with pytest.raises(sa.SuffixArrayError):
        sa.DeviceIndex.infgram_score(None, b"abc", doc_offsets=[[0, 3]])


def test_group_cap_switch():
    try:
        assert sa.score_set_group_cap(100) == sa.SCORE_GROUP_CAP_DEFAULT
        assert sa.score_set_group_cap(0) == 100
        assert sa.score_set_group_cap(2**40) == 0                      # a huge value is clamped, not refused
        assert sa.score_set_group_cap(-1) == 1 << 20
        assert sa.score_set_group_cap(-7) == 64
    finally:
        sa.score_set_group_cap(-1)
