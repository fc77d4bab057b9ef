"""CPU suite for the Burrows-Wheeler transform and its inverse: the definition and the three-phase inverse of kernels/bwt.hpp
restated in numpy (hashed splitters, walk cap and resume, restart with denser splitters, pointer-jumping ranks) and pinned
against the literal walk; the exports; the argument checks that answer without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases, fibonacci_word

EXPORTS = ("sa_amd_bwt", "sa_amd_bwt_device", "sa_amd_bwt_work_bytes", "sa_amd_index_bwt", "sa_amd_unbwt", "sa_amd_unbwt_device",
           "sa_amd_unbwt_work_bytes", "sa_amd_last_unbwt_stats", "sa_amd_unbwt_set_walk_limits", "sa_amd_unbwt_set_splitter_spacing")
PY_NAMES = ("bwt", "unbwt", "bwt_device_ptr", "unbwt_device_ptr", "bwt_work_bytes", "unbwt_work_bytes", "last_unbwt_stats",
            "unbwt_set_walk_limits", "unbwt_set_splitter_spacing", "UnbwtStats")

# the issue's table, computed with a numpy restatement of the definition over the oracle's SA-IS
KNOWN = [
    (b"banana", b"annbaa", 4), (b"mississippi", b"ipssmpissii", 5), (b"a", b"a", 1), (b"ab", b"ba", 1), (b"aa", b"aa", 2),
    (b"\xff\x00\xff", b"\xff\xff\x00", 3), (b"", b"", 0),
]

SPACING_DEFAULT, SPACING_MIN, RESTART_WALKS = 256, 4, 64      # host/tuning.hpp


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(0, dtype=np.uint8)


def bwt_definition(t, arr):
    """(B, primary) of the contract in include/suffix_array_amd.h, from the text and its suffix array (arr[0] == n)"""
    n = t.size
    if n == 0:
        return np.zeros(0, dtype=np.uint8), 0
    s = np.asarray(arr).astype(np.int64)
    primary = int(np.nonzero(s == 0)[0][0])
    rows = np.delete(s, primary)
    return t[rows - 1], primary


def psi_and_first_column(b, primary):
    """phase 1: ψ[k + 1] = row(order[k]), ψ[0] = primary; F[k + 1] = b[order[k]] (F[0] is the sentinel's row)"""
    n = b.size
    order = np.argsort(b, kind="stable").astype(np.int64)
    psi = np.empty(n + 1, dtype=np.int64)
    psi[0] = primary
    psi[1:] = np.where(order < primary, order, order + 1)
    first = np.zeros(n + 1, dtype=np.uint8)
    first[1:] = b[order]
    return psi, first


def literal_inverse(b, primary):
    """the plain walk: T[j] = F[ψ^j(primary)]; None when the walk from primary closes before it has visited n + 1 rows"""
    n = b.size
    if n == 0:
        return np.zeros(0, dtype=np.uint8) if primary == 0 else None
    if not 1 <= primary <= n:
        return None
    psi, first = psi_and_first_column(b, primary)
    out = np.zeros(n, dtype=np.uint8)
    row = primary
    for j in range(n):
        if row == 0:
            return None                                   # row 0 leads back to primary: closed after j + 1 < n + 1 rows
        out[j] = first[row]
        row = int(psi[row])
    return out if row == 0 else None


def row_hash(row, seed):
    """unbwt_hash of kernels/bwt.hpp: two rounds of multiply - xorshift"""
    h = (row + seed * 0x9E3779B9) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def row_hash_np(rows, seed):
    h = (rows.astype(np.uint64) + np.uint64((seed * 0x9E3779B9) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def splitter_mask(n, primary, spacing, seed, hashed=True):
    rows = np.arange(n + 1, dtype=np.int64)
    m = (row_hash_np(rows, seed) & np.uint64(spacing - 1)) == 0 if hashed else rows % spacing == 0
    m[primary] = True
    return m


def three_phase_inverse(b, primary, spacing=SPACING_DEFAULT, cap=None, max_launches=None):
    """host/bwt.hpp in numpy.  Returns (text or None, stats)."""
    n = b.size
    stats = {"walkers": 0, "steps": 0, "longest_walk": 0, "splitter_spacing": 0, "walk_launches": 0, "restarts": 0}
    if n == 0:
        return (np.zeros(0, dtype=np.uint8) if primary == 0 else None), stats
    if not 1 <= primary <= n:
        return None, stats
    psi, first = psi_and_first_column(b, primary)
    cap = 4096 if cap is None else max(cap, 1)
    seed = 0
    while True:
        is_split = splitter_mask(n, primary, spacing, seed)
        srow = np.nonzero(is_split)[0]
        m = srow.size
        widx = np.full(n + 1, -1, dtype=np.int64)
        widx[srow] = np.arange(m)
        last_try = spacing <= SPACING_MIN
        limit = max_launches if max_launches and max_launches > 0 else -(-RESTART_WALKS * spacing // cap)
        state = [(int(r), 0) for r in srow]              # (row, steps so far); None when the walker has arrived
        nxt, length = np.full(m, -1, dtype=np.int64), np.zeros(m, dtype=np.int64)
        active, launches = m, 0
        while active and (last_try or launches < limit):
            active = 0
            for w in range(m):
                if state[w] is None:
                    continue
                row, steps = state[w]
                there = False
                for _ in range(cap):
                    row = int(psi[row])
                    steps += 1
                    stats["steps"] += 1
                    if is_split[row]:
                        there = True
                        break
                if there:
                    nxt[w] = -1 if row == primary else widx[row]     # the list is cut in front of primary's walker
                    length[w] = steps
                    state[w] = None
                else:
                    state[w] = (row, steps)                         # resumed, never started over
                    active += 1
            launches += 1
        stats["walk_launches"] += launches
        if not active:
            break
        stats["restarts"] += 1
        spacing = max(spacing // 8, SPACING_MIN)
        seed += 1
    stats.update(walkers=m, splitter_spacing=spacing, longest_walk=int(length.max()))
    # pointer jumping, ceil(log2 m) rounds
    d = length.copy()
    for _ in range(int(m - 1).bit_length()):
        live = nxt >= 0
        d2, n2 = d.copy(), nxt.copy()
        d2[live] = d[live] + d[nxt[live]]
        n2[live] = nxt[nxt[live]]
        d, nxt = d2, n2
    p = int(widx[primary])
    if d[p] != n + 1 or nxt[p] != -1:
        return None, stats
    base = d[p] - d
    out = np.zeros(n, dtype=np.uint8)
    for w in range(m):
        row, j = int(srow[w]), int(base[w])
        while True:
            if row != 0 and j < n:
                out[j] = first[row]
            row = int(psi[row])
            j += 1
            stats["steps"] += 1
            if is_split[row]:
                break
    return out, stats


def invalid_pair(n, seed):
    """(b, primary) of n bytes whose walk from primary closes early: seeded bytes of four values (the row permutation of such a
    string nearly always falls into several cycles) and the first primary whose cycle is shorter than n + 1 rows"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 4, n, dtype=np.uint8)
    for primary in range(1, n + 1):
        if literal_cycle_length(b, primary) != n + 1:
            return b, primary
    raise AssertionError("no invalid pair found")


def literal_cycle_length(b, primary):
    psi, _ = psi_and_first_column(b, primary)
    row, k = int(psi[primary]), 1
    while row != primary:
        row = int(psi[row])
        k += 1
    return k


def longest_gap(b, primary, spacing, hashed):
    """longest walk between neighbouring splitters (vectorised: all walkers step together)"""
    psi, _ = psi_and_first_column(b, primary)
    is_split = splitter_mask(b.size, primary, spacing, 0, hashed)
    cur = psi[np.nonzero(is_split)[0]]
    steps = 1
    while True:
        cur = cur[~is_split[cur]]
        if cur.size == 0:
            return steps
        cur = psi[cur]
        steps += 1


# ---------------------------------------------------------------------------------------------------------------------


def test_definition_on_known_answers(oracle):
    for text, exp_b, exp_p in KNOWN:
        t = _u8(text)
        b, p = bwt_definition(t, oracle.sais(t))
        assert (b.tobytes(), p) == (exp_b, exp_p), text
        assert literal_inverse(_u8(exp_b), exp_p).tobytes() == text


@pytest.mark.parametrize("cap", [1, 2, 3, None])
def test_three_phase_model_matches_the_literal_walk(oracle, cap):
    texts = [_u8(b) for b in adversarial_cases().values()] + [_u8(k[0]) for k in KNOWN]
    rng = np.random.default_rng(11)
    for k in range(30):
        texts.append(rng.integers(0, [2, 4, 26, 256][k % 4], int(rng.integers(1, 3000)), dtype=np.uint8))
    for t in texts:
        b, p = bwt_definition(t, oracle.sais(t))
        lit = literal_inverse(b, p)
        assert lit is not None and np.array_equal(lit, t)
        # small spacing: many walkers on short texts; with cap 1..3 every walk is resumed over several launches
        got, st = three_phase_inverse(b, p, spacing=16, cap=cap, max_launches=1 << 30)
        assert got is not None and np.array_equal(got, t)
        assert st["restarts"] == 0
        assert st["steps"] == (2 * (t.size + 1) if t.size else 0)        # each row once per walking phase: a resumed walk never starts over
        if cap is not None and t.size > 64:
            assert st["walk_launches"] > 1


def test_three_phase_model_restart_path(oracle):
    t = np.frombuffer(fibonacci_word(16), dtype=np.uint8)
    b, p = bwt_definition(t, oracle.sais(t))
    got, st = three_phase_inverse(b, p, spacing=256, cap=2, max_launches=3)
    assert np.array_equal(got, t)
    assert st["restarts"] >= 1 and st["splitter_spacing"] < 256
    got, st = three_phase_inverse(b, p, spacing=256, cap=1, max_launches=1)     # down to the densest set, which has no launch limit
    assert np.array_equal(got, t) and st["splitter_spacing"] == SPACING_MIN and st["restarts"] == 2


def test_model_refuses_pairs_whose_walk_closes_early():
    assert literal_inverse(_u8(b"ba"), 2) is None
    for cap in (1, 3, None):
        assert three_phase_inverse(_u8(b"ba"), 2, cap=cap)[0] is None
    assert three_phase_inverse(_u8(b"ba"), 1)[0].tobytes() == b"ab"
    for n, seed in ((7, 1), (100, 2), (1000, 3)):
        b, p = invalid_pair(n, seed)
        assert literal_inverse(b, p) is None
        for spacing, cap in ((4, 1), (16, None), (256, 5)):
            assert three_phase_inverse(b, p, spacing=spacing, cap=cap, max_launches=1 << 30)[0] is None
    for primary in (0, 3, -1):
        assert three_phase_inverse(_u8(b"ba"), primary)[0] is None


def test_hashed_splitters_spread_where_row_numbers_do_not(oracle):
    """DESIGN.md section 12's table at a size the CPU suite can afford (n = 2^16, S = 64): `row % S` leaves one walker a large
    part of text ++ text and of the repeated ramp; hashed rows stay below 32 S on every family"""
    n, spacing = 1 << 16, 64
    rng = np.random.default_rng(5)
    half = rng.integers(0, 256, n // 2, dtype=np.uint8)
    fib = fibonacci_word(24)
    families = {
        "random": rng.integers(0, 256, n, dtype=np.uint8), "one_byte": np.full(n, 7, dtype=np.uint8),
        "period2": np.tile(np.array([1, 2], dtype=np.uint8), n // 2), "fibonacci": np.frombuffer(fib[:n], dtype=np.uint8),
        "twice": np.concatenate([half, half]), "ramp_rep": np.tile(np.arange(256, dtype=np.uint8), n // 256),
    }
    plain = {}
    for name, t in families.items():
        b, p = bwt_definition(t, oracle.sais(t))
        assert longest_gap(b, p, spacing, True) <= 32 * spacing, name
        plain[name] = longest_gap(b, p, spacing, False)
    assert plain["twice"] > 32 * spacing and plain["ramp_rep"] > 32 * spacing, plain


def test_header_python_and_library_name_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "suffix_array_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sa_amd_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert fn in declared, fn
        assert hasattr(L, fn), fn
    assert "sa_amd_unbwt_stats" in src
    for name in PY_NAMES:
        assert name in sa.__all__, name
        assert hasattr(sa, name), name
    assert callable(sa.DeviceIndex.bwt) and callable(sa.SuffixArray.bwt)
    assert ctypes.sizeof(sa.UnbwtStats) == 40


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.zeros(16, dtype=np.uint32)
    p = buf.ctypes.data
    prim = ctypes.c_int32(7)
    assert L.sa_amd_bwt_work_bytes(-1) == -1 and L.sa_amd_unbwt_work_bytes(-1) == -1
    assert L.sa_amd_bwt(None, -1, p, p, ctypes.byref(prim)) == -1                 # n < 0
    assert L.sa_amd_bwt(None, 4, p, p, ctypes.byref(prim)) == -1                  # null text
    assert L.sa_amd_bwt(p, 4, p, None, ctypes.byref(prim)) == -1                  # null output
    assert L.sa_amd_bwt(p, 4, p, p, None) == -1                                   # nowhere to put primary
    assert L.sa_amd_bwt_device(p, p, -1, p, ctypes.byref(prim), p, 256, None) == -1
    assert L.sa_amd_bwt_device(p, None, 4, p, ctypes.byref(prim), p, 256, None) == -1
    assert L.sa_amd_bwt_device(None, p, 4, p, ctypes.byref(prim), p, 256, None) == -1
    assert L.sa_amd_bwt_device(p, p, 4, None, ctypes.byref(prim), p, 256, None) == -1
    assert L.sa_amd_bwt_device(p, p, 4, p, None, p, 256, None) == -1
    assert L.sa_amd_bwt_device(p, p, 4, p, ctypes.byref(prim), None, 256, None) == -1
    assert L.sa_amd_index_bwt(None, p, ctypes.byref(prim)) == -1
    assert L.sa_amd_unbwt(None, -1, 0, p) == -1
    assert L.sa_amd_unbwt(None, 4, 1, p) == -1
    assert L.sa_amd_unbwt(p, 4, 1, None) == -1
    for bad in (0, 5, -1):
        assert L.sa_amd_unbwt(p, 4, bad, p) == -1                                 # primary outside 1 .. n: refused before any device work
        with pytest.raises(ValueError):
            sa.unbwt(b"abcd", bad)
    assert L.sa_amd_unbwt(None, 0, 1, None) == -1                                 # the empty string's primary is 0
    assert L.sa_amd_unbwt_device(p, -1, 0, p, p, 1 << 20, None) == -1
    assert L.sa_amd_unbwt_device(None, 4, 1, p, p, 1 << 20, None) == -1
    assert L.sa_amd_unbwt_device(p, 4, 1, None, p, 1 << 20, None) == -1
    assert L.sa_amd_unbwt_device(p, 4, 1, p, None, 1 << 20, None) == -1
    assert prim.value == 7
    st = sa.UnbwtStats()
    L.sa_amd_last_unbwt_stats(ctypes.byref(st))                                   # (no transform on this thread yet: zeros)
    L.sa_amd_last_unbwt_stats(None)
    assert sa.last_unbwt_stats()["restarts"] == 0
    sa.unbwt_set_walk_limits(1, 1)                                                # (thread-local route switches: no device involved)
    sa.unbwt_set_walk_limits(-1, -1)
    assert sa.unbwt_set_splitter_spacing(100) == 256                              # rounded down to a power of two, clamped to 4 .. 65 536
    assert sa.unbwt_set_splitter_spacing(1) == 64
    assert sa.unbwt_set_splitter_spacing(1 << 30) == 4
    assert sa.unbwt_set_splitter_spacing(-1) == 65536
    assert sa.unbwt_set_splitter_spacing(-1) == 256


@pytest.mark.parametrize("n", [0, 1, 2, 1000, 4096, 1 << 20, (1 << 30) + 4097, 2**31 - 1])
def test_work_blocks(n):
    """the inverse's work block is no larger than the LCP array's plus the slab of the 257 digit starts (which only shows on
    texts of a few bytes); the forward one is the control slab"""
    L = sa.lib()
    w = L.sa_amd_unbwt_work_bytes(n)
    assert 0 < w <= L.sa_amd_lcp_work_bytes(n) + 1280
    if n >= 4096:
        assert w <= 17 * (n + 1) + (2 << 20)
    assert w % 256 == 0
    assert L.sa_amd_bwt_work_bytes(n) == 256
    # the walker tables (five words per walker in two (n + 1)-entry buffers) hold the densest splitter set with room to spare
    if n >= 1000:
        cap_walkers = (2 * ((n + 1 + 67) & ~3)) // 5
        assert cap_walkers >= 1.5 * (n + 1) / SPACING_MIN
