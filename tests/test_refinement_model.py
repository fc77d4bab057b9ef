"""The numpy model of the refinement rounds (tests/refinement_model.py) against independent references, on the CPU: brute-force
window classes, the oracle's suffix array and its Kasai LCP array, the closed form of the Fibonacci word, and a trace recorded
on the MI355X.  tests/test_refinement_rounds.py holds real builds to this model round by round, so it must not be the weakest
link."""
import ast
import ctypes
import functools
import os

import numpy as np
import pytest

import refinement_model as rm
from conftest import adversarial_cases, fibonacci_word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 7, 8, 13, 64]


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _texts():
    out = {name: _u8(b) for name, b in adversarial_cases().items()}
    rng = np.random.default_rng(2024)
    for sigma in (2, 4, 57, 256):
        for n in (1, 2, 63, 997, 5000):
            out[f"random_s{sigma}_n{n}"] = rng.integers(0, sigma, n, dtype=np.uint8) + np.uint8(0 if sigma == 256 else 40)
    body = rng.integers(0, 4, 3000, dtype=np.uint8) + np.uint8(65)
    # the smallest byte in a run at the end (padding collides with it), only in the middle, and both
    out["low_run_at_end"] = np.concatenate([body, np.full(200, 65, dtype=np.uint8)])
    out["low_run_at_end_s57"] = np.concatenate([rng.integers(1, 57, 2000, dtype=np.uint8), np.zeros(130, dtype=np.uint8)])
    out["low_run_in_middle"] = np.concatenate([body[:1500] | np.uint8(1), np.full(200, 64, dtype=np.uint8), body[1500:] | np.uint8(1)])
    out["low_run_middle_and_end"] = np.concatenate([body[:1000], np.full(90, 65, dtype=np.uint8), body[1000:2000], np.full(70, 65, dtype=np.uint8)])
    return out


def _brute_force_classes(t, k):
    """classes of the rows of the n x k matrix of padded windows, by np.unique"""
    n = t.size
    e = np.concatenate([rm.codes(t), np.zeros(k, dtype=np.int64)])
    win = np.lib.stride_tricks.sliding_window_view(e, k)[:n]
    _, inv = np.unique(win, axis=0, return_inverse=True)
    return np.asarray(inv).reshape(-1) + 1


def _inverse(oracle, t):
    arr = oracle.sais(t)[1:].astype(np.int64)
    inv = np.empty(t.size, dtype=np.int64)
    inv[arr] = np.arange(t.size)
    return inv


def _kasai(oracle, t):
    L = oracle.L
    L.oracle_lcp_kasai.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.oracle_lcp_kasai.restype = ctypes.c_int32
    arr = oracle.sais(t)
    out = np.zeros(t.size + 1, dtype=np.uint32)
    assert L.oracle_lcp_kasai(t.ctypes.data, t.size, arr.ctypes.data, out.ctypes.data) == 0
    return out.astype(np.int64)


@pytest.mark.parametrize("k", KS)
def test_initial_classes_equal_brute_force(k):
    for name, t in _texts().items():
        if t.size == 0:
            assert rm.initial(t, k).size == 0 and rm.tied(rm.initial(t, k)) == 0
            continue
        got = rm.initial(t, k)
        assert np.array_equal(got, _brute_force_classes(t, k)), (name, k)


def test_padding_ties_a_short_suffix_with_a_longer_one():
    """the property the brute force shares with the model by construction, pinned by hand: "ab" + "aaa": the suffixes a, aa,
    aaa and (depth 2) nothing else tie under zero padding; b"ba": nothing ties"""
    t = _u8(b"abaaa")
    assert rm.initial(t, 1).tolist() == [1, 2, 1, 1, 1]
    assert rm.initial(t, 2).tolist() == [2, 3, 1, 1, 1]              # aa, a0 -> (0, 0) with a = code 0
    assert rm.tied(rm.initial(t, 2)) == 3 and rm.tied(rm.initial(t, 64)) == 3
    assert rm.tied(rm.initial(_u8(b"ba"), 64)) == 0
    assert rm.tied(np.array([1, 1, 2, 3, 3, 3, 4])) == 5 and rm.tied(np.zeros(0, dtype=np.int64)) == 0


@pytest.mark.parametrize("k,s", [(1, 1), (2, 5), (7, 6), (8, 8), (13, 51), (64, 23)])
def test_a_text_round_is_the_initial_classes_of_the_sum(k, s):
    for name, t in _texts().items():
        if t.size:
            assert np.array_equal(rm.text_round(rm.initial(t, k), t, k, s), rm.initial(t, k + s)), (name, k, s)


@pytest.mark.parametrize("iters,factor", [(1, 2), (3, 4)])
def test_rank_rounds_end_at_the_inverse_suffix_array(oracle, iters, factor):
    """pins the past-the-end rule and the order of the ids: every class single, cls - 1 the oracle's inverse"""
    for name, t in _texts().items():
        if t.size == 0:
            continue
        cls, h = rm.initial(t, 1), 1
        before = rm.tied(cls)
        while h < t.size:
            cls = rm.rank_round(cls, h, iters)
            now = rm.tied(cls)
            assert now <= before, (name, h)
            before = now
            h *= factor
        assert rm.tied(cls) == 0, name
        assert np.array_equal(cls - 1, _inverse(oracle, t)), name


def test_rank_rounds_from_padded_keys_end_at_the_inverse_suffix_array(oracle):
    """the library's own start: 64 padded symbols, then offsets 64, 128, ... -- the padding's ties come apart in the first
    round (every member but the longest reads past the end)"""
    for name, t in _texts().items():
        if t.size == 0:
            continue
        cls, h = rm.initial(t, 64), 64
        while rm.tied(cls):
            assert h < 64 * 2 * max(t.size, 1), name
            cls = rm.rank_round(cls, h, 1)
            h *= 2
        assert np.array_equal(cls - 1, _inverse(oracle, t)), name


def test_one_chasing_round_equals_its_single_rounds_in_tied_count():
    """iters look-ups at h refine to (iters + 1) h symbols: at least as fine as one look-up, and on a text without padding
    collisions exactly the classes of that depth"""
    rng = np.random.default_rng(5)
    t = np.concatenate([[0], np.resize(rng.integers(1, 5, 300, dtype=np.uint8), 4000)]).astype(np.uint8)
    base = rm.initial(t, 8)
    for iters in (2, 3, 7):
        chased = rm.rank_round(base, 8, iters)
        assert rm.tied(chased) <= rm.tied(rm.rank_round(base, 8, 1))
        assert rm.tied(chased) == rm.tied(rm.initial(t, 8 * (iters + 1))), iters


def test_a_chase_that_stops_one_look_up_early_moves_the_counts_but_not_the_array(oracle):
    """why the rounds are checked one by one: I - 1 look-ups where the host assumes I (and multiplies h by I + 1) skip h symbols
    per round.  In a repeated block two tied suffixes differ only where the shorter one ends, which every later look-up still
    finds: the finished array is the oracle's, and only the tied counts tell"""
    t = np.tile(np.random.default_rng(8).integers(0, 256, 70, dtype=np.uint8), 97)
    right, early, h = rm.initial(t, 8), rm.initial(t, 8), 8
    differed = 0
    while rm.tied(right) or rm.tied(early):
        right, early, h = rm.rank_round(right, h, 3), rm.rank_round(early, h, 2), 4 * h
        assert rm.tied(early) >= rm.tied(right)
        differed += rm.tied(early) != rm.tied(right)
    assert differed >= 2
    assert np.array_equal(early, right) and np.array_equal(early - 1, _inverse(oracle, t))


@pytest.mark.parametrize("seed,sigma,n", [(1, 2, 5000), (2, 4, 4097), (3, 56, 5000), (4, 255, 3000)])
def test_unpadded_depth_equals_the_lcp_array(oracle, seed, sigma, n):
    """bytes >= 1 behind one leading 0: the smallest byte never sits where zero padding could collide with it, so the suffixes
    tied at depth d are those with a neighbour in the suffix array that shares d symbols"""
    rng = np.random.default_rng(seed)
    block = rng.integers(1, sigma + 1, max(n // 7, 1), dtype=np.uint8)
    body = np.concatenate([np.resize(block, n // 2), rng.integers(1, sigma + 1, n - 1 - n // 2, dtype=np.uint8)])
    t = np.concatenate([np.zeros(1, dtype=np.uint8), body]).astype(np.uint8)
    lcp = np.concatenate([_kasai(oracle, t), [0]])          # lcp[r]: slots r - 1 and r of the (n + 1)-entry array; lcp[n + 1] = 0
    reach = np.maximum(lcp[1:-1], lcp[2:])                   # per real suffix (slots 1 .. n)
    for d in (1, 2, 3, 7, 8, 13, 64, 65, 128, 700):
        assert rm.tied(rm.initial(t, d)) == int((reach >= d).sum()), d
    cls, h = rm.initial(t, 8), 8
    while h < 2 * n:
        cls = rm.rank_round(cls, h, 1)
        h *= 2
        assert rm.tied(cls) == int((reach >= h).sum()), h


@pytest.mark.parametrize("n", [70_001, 1 << 16])
def test_fibonacci_prefix_follows_its_closed_form(n):
    """a prefix of the Fibonacci word has d + 1 factors of every length d, each repeated all over it: only the last d - 1
    suffixes are alone at depth d.  "While h is small against n": a factor of length d recurs in every window of
    F(k+3) + d - 1 < 5.3 d symbols (F(k) <= d, the recurrence function of the Fibonacci word), so it starts twice among the
    first n - d positions once n >= 12 d.
    Exact where padding cannot collide (the letters as codes 1 and 2 behind one leading 0, which is alone from depth 1 on).
    With a as code 0 the 63 padded tails may equal real factors or each other, and a suffix that looks such a tail up inherits
    the tie for a round: the counts then depend on how the prefix ends (next test), which is what the model is for."""
    t = np.concatenate([np.zeros(1, dtype=np.uint8), _u8(fibonacci_word(26)[:n - 1]) - np.uint8(96)])
    m = n - 1
    cls, h = rm.initial(t, 64), 64
    assert rm.tied(cls) == m - 63
    while 12 * 2 * h <= m:
        cls = rm.rank_round(cls, h, 1)
        h *= 2
        assert rm.tied(cls) == m - (h - 1), h
    assert h >= 2048
    h //= 4                                                  # the same depth by a chase from a quarter of it
    assert rm.tied(rm.rank_round(rm.initial(t, h), h, 3)) == m - (4 * h - 1)


def test_fibonacci_keys_leave_n_minus_61_tied_at_a_power_of_two():
    """what the recorded build of 2^28 bytes reports (profiles/r02_round_trace_adv_fib_268435456.txt), on prefixes that end
    in the same letters (baa), and n - (h - 1) after the rounds that follow, as recorded"""
    for n in (1 << 16, 1 << 20):
        t = _u8(fibonacci_word(28)[:n])
        assert bytes(t[-3:]) == b"baa"
        cls = rm.initial(t, 64)
        assert rm.tied(cls) == n - 61
        if n == 1 << 16:
            for h in (64, 128, 256, 512, 1024):
                cls = rm.rank_round(cls, h, 1)
                assert rm.tied(cls) == n - (2 * h - 1), h


def test_parser_reads_the_recorded_fibonacci_trace_without_loss():
    """recorded numbers, not a GPU run: 2^28 bytes of the Fibonacci word, dense from the start"""
    n = 268435456
    path = os.path.join(ROOT, "profiles", "r02_round_trace_adv_fib_268435456.txt")
    text = open(path).read()
    rounds = rm.parse_trace(text)
    assert [r["kind"] for r in rounds] == ["done"] + ["doubling"] * 18
    assert text.count("doubling round") == 18 and ": text round" not in text
    stats = ast.literal_eval(text[text.index("stats {") + 6:].strip())
    assert (stats["rounds"], stats["unresolved_after_initial"], stats["text_rounds"], stats["symbols_per_key"]) == (18, n - 61, 0, 64)
    assert rounds[0]["m"] == n - 61
    h, m = 64, rounds[0]["m"]
    for number, r in enumerate(rounds[1:], start=1):
        assert r["round"] == number and r["mode"] == "dense"
        assert r["h"] == h and r["a"] == m, r
        h, m = rm.next_h(h, r["iters"], r["m_global"]), r["b"]
        if 12 * h <= n:                                      # (rounds 1 .. 16; see test_fibonacci_prefix_follows_its_closed_form)
            assert number <= 16
            assert r["b"] == n - (h - 1), r
        assert r["written"] >= 0
    assert m == 0
    assert [r["iters"] for r in rounds[1:]] == [1] * 14 + [3] * 4
    assert [r["m_global"] > 0 for r in rounds[1:]] == [True] * 13 + [False] * 5


def test_parser_reads_text_and_sparse_lines():
    text = ("suffix_array_amd: text round 1 depth 19: tied 1000 -> 400  (0.12 ms)\n"
            "noise\nsuffix_array_amd: text round 2 depth 25: tied 400 -> 30  (0.10 ms)\n"
            "suffix_array_amd: initial sort + text rounds + rank set-up done, 30 tied (0.05 ms since the last line)\n"
            "suffix_array_amd: doubling round 3 h 25 (sparse, 1 look-ups, 0 through the global sort): tied 30 -> 0, -1 ranks written\n"
            "    (0.07 ms)\n")
    assert rm.parse_trace(text) == [
        {"kind": "text", "round": 1, "depth": 19, "a": 1000, "b": 400}, {"kind": "text", "round": 2, "depth": 25, "a": 400, "b": 30},
        {"kind": "done", "m": 30},
        {"kind": "doubling", "round": 3, "h": 25, "mode": "sparse", "iters": 1, "m_global": 0, "a": 30, "b": 0, "written": -1}]
    assert rm.next_h(64, 1, 0) == 128 and rm.next_h(64, 3, 0) == 256 and rm.next_h(64, 3, 5) == 128 and rm.next_h(64, 1, 9) == 128
