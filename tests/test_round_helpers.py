"""The helper kernels of a refinement round.

k_rr_count, byte forms (kernels/rerank.hpp): a lane holds the bytes of eight consecutive members and counts on its own eight
bits (rr_wave_count_bits) -- tied members from the lane's boundary bits and bit 0 of the next lane's, the wave's last and first
group start from one ballot and three v_readlane.  A lane is 8 members, a wave 512, a tile 8 192, a span of tiles 32 768.

The set-up's two scans run as the two blocks of one launch (k_rr_scan_round, host/pipeline.hpp): every dense build below
passes through it.

1. the lane-local formulas restated in numpy, against the mask form (what k_rr_apply still computes) on random bytes: no GPU;
2. whole builds on texts whose lists put group starts on the ends of lanes, waves, tiles and spans: every array is the
   oracle's, statistics and per-round tied counts are those of the key route of the diagnostic library (rf._check), as in
   test_round_flags.py, test_head_flags.py and test_rerank_spans.py, whose generators and build helpers are used here."""
import ctypes
import functools

import numpy as np
import pytest

import suffix_array_amd as sa
import refinement_model as rm
import test_head_flags as hf
import test_round_flags as rf

LANE, WAVE_MEMBERS, RR_TILE, SPAN = 8, 512, 8192, 32768
DENSE = {"SA_AMD_FORCE_DENSE": "1"}
GENERAL = dict(DENSE, SA_AMD_SMALL_MAX="0")      # (a text of up to 8 192 bytes: through the general pipeline, not the one-workgroup build)
RS_KEYED, RS_HEAD, RS_PHEAD = 2, 4, 8
NO_HEAD = 0xFFFFFFFF


# ---- 1. the formulas ---------------------------------------------------------------------------------------------------------

def _mask_form(head, phead, valid, after, wbase):
    """(tied members, list index of the last group start + 1, head code of the first one) of one wave from its 512 head / parent
    head / valid bits in list order and the boundary bit of the member behind the wave"""
    bnd = head | ~valid
    nxt = np.concatenate([bnd[1:], [after]])
    tied = valid & ~(head & nxt)
    at = np.flatnonzero(head)
    if at.size == 0:
        return int(tied.sum()), 0, NO_HEAD
    return int(tied.sum()), wbase + int(at[-1]) + 1, ((wbase + int(at[0])) << 1) | int(phead[at[0]])


def _lane_form(hb, pb, vb, after, wbase):
    """the same from the 64 lanes' bytes hb, pb, vb (bit k of lane l: member 8 l + k), as rr_wave_count_bits does it"""
    hb, pb, vb = (x.astype(np.uint32) for x in (hb, pb, vb))
    b = (hb | ~vb) & 255
    nb = np.concatenate([b[1:] & 1, [1 if after else 0]]).astype(np.uint32)
    tied = vb & ~(hb & ((b >> 1) | (nb << 7)))
    cnt = sum(int(((tied >> k) & 1).sum()) for k in range(LANE))
    lanes = np.flatnonzero(hb)
    if lanes.size == 0:
        return cnt, 0, NO_HEAD
    top, low = int(lanes[-1]), int(lanes[0])
    msb = int(hb[top]).bit_length() - 1
    lsb = (int(hb[low]) & -int(hb[low])).bit_length() - 1
    return cnt, wbase + LANE * top + msb + 1, ((wbase + LANE * low + lsb) << 1) | ((int(pb[low]) >> lsb) & 1)


def _pack(bits):
    return np.packbits(bits.reshape(-1, LANE), axis=1, bitorder="little").reshape(-1)


def test_lane_local_formulas_against_the_mask_form():
    rng = np.random.default_rng(20240607)
    densities = [0.0, 0.002, 0.05, 0.5, 0.95, 1.0]
    lengths = [WAVE_MEMBERS] * 6 + [0, 1, 7, 8, 9, 63, 64, 65, 255, 504, 505, 511]
    cases = 0
    for density in densities:
        for left in lengths:
            for after in (False, True):
                for _ in range(4):
                    valid = np.arange(WAVE_MEMBERS) < left
                    # status bytes and keys of a dense round; a group starts at  PHEAD || (KEYED ? key differs : HEAD)
                    status = rng.integers(0, 16, WAVE_MEMBERS, dtype=np.uint8)
                    status[rng.random(WAVE_MEMBERS) >= density] &= np.uint8(~(RS_HEAD | RS_PHEAD) & 255)
                    keys = rng.integers(0, 3 if density < 0.9 else 1000, WAVE_MEMBERS + 1)
                    differs = keys[1:] != keys[:-1]
                    phead = (status & RS_PHEAD) != 0
                    head = phead | np.where((status & RS_KEYED) != 0, differs & (rng.random(WAVE_MEMBERS) < max(density, 0.01)), (status & RS_HEAD) != 0)
                    head &= valid
                    phead &= valid
                    behind = after or left < WAVE_MEMBERS          # (the list ends inside the wave: the kernel passes a boundary)
                    wbase = int(rng.integers(0, 1 << 18)) * WAVE_MEMBERS
                    want = _mask_form(head, phead, valid, behind, wbase)
                    got = _lane_form(_pack(head), _pack(phead), _pack(valid), behind, wbase)
                    assert got == want, (density, left, after)
                    cases += 1
    # ... and the shapes a random draw seldom makes: one start per lane position, alone in the wave
    for at in list(range(0, 17)) + [255, 256, 503, 504, 510, 511]:
        for after in (False, True):
            head = np.zeros(WAVE_MEMBERS, dtype=bool)
            head[at] = True
            valid = np.ones(WAVE_MEMBERS, dtype=bool)
            assert _lane_form(_pack(head), _pack(head), _pack(valid), after, 4096) == _mask_form(head, head, valid, after, 4096), (at, after)
    assert cases > 500


# ---- 2. whole builds ---------------------------------------------------------------------------------------------------------

def _first_doubling(err):
    return [r for r in rm.parse_trace(err) if r["kind"] == "doubling"][0]


def _pairs_text(m, k, salt):
    """A text whose tied list behind an initial sort on k symbols has exactly m members: random bytes above 0, one block of
    pairs + k - 1 of them copied twice -- a pair of tied suffixes for every offset that leaves k bytes of the block, so every
    second place of the list starts a group -- and, for an odd m, k zero bytes copied three times: the triple is the smallest
    group, in front of the list, and the pairs behind it start on the odd places."""
    pairs = (m - 3) // 2 if m % 2 else m // 2
    seed = 1_000_000 * salt + m
    rnd = lambda s, c: rf._rnd(s + seed, c, 1, 256)          # noqa: E731
    B = rnd(11, pairs + k - 1)
    parts = [rnd(12, 3000), B, rnd(13, 1500), B, rnd(14, 2500)]
    if m % 2:
        C = np.zeros(k, dtype=np.uint8)
        for j in range(3):      # (the bytes around the copies differ, so that no window that leaves the block is tied)
            parts += [np.array([10 + j], dtype=np.uint8), C, np.array([40 + j], dtype=np.uint8), rnd(15 + j, 500 + 100 * j)]
    return np.concatenate(parts)


def _text_with_a_list_of(monkeypatch, capfd, m):
    """the key of the initial sort holds fewer symbols on longer texts: the first doubling round of a key-route build says how
    many it held and how long the list is, and the text is made again until both fit (as in test_rerank_spans.py)"""
    k = rf.KEY_SYMBOLS
    for salt in range(6):
        t = _pairs_text(m, k, salt)
        first = _first_doubling(rf._build(monkeypatch, capfd, GENERAL, t, 0)[2])
        if first["h"] == k and first["a"] == m:
            return t
        k = first["h"]
    raise AssertionError((m, first))


# Pairs from place 0 put group starts on the even places -- 8, 512, 8 192, 32 768 --, pairs behind a triple on 0 and the odd
# places from 3 -- 7 and 9, 511 and 513, 8 191 and 8 193, 32 767 and 32 769 -- and a pair across every lane, wave, tile and span
# end (places 2 047 and 2 048 also straddle a tile of k_group_sort: KEYED places, a run from a lane's last member to the next
# lane's first).  The lengths: m = 1 .. 7 (mod 8) around a tile and around a span, and lists that end a few members behind
# the first lane, wave, tile and span.
PAIR_LISTS = sorted({8192 + r for r in range(1, 8)} | {32768 + r for r in range(1, 8)} | {10, 11, 514, 515, 8192, 32768, 32778, 32779})


def _list_groups(exp, t, k):
    """the group (class of the first k symbols) of every place of the tied list behind the initial sort, from the oracle's array"""
    c = rm.initial(t, k)[exp[1:].astype(np.int64)]          # (exp[0] is the sentinel)
    same = c[1:] == c[:-1]
    tied = np.zeros(c.size, dtype=bool)
    tied[1:] |= same
    tied[:-1] |= same
    return c[tied]


@pytest.mark.gpu
@pytest.mark.parametrize("m", PAIR_LISTS)
def test_lists_of_pairs(oracle, monkeypatch, capfd, m):
    name, t = f"helpers_pairs_{m}", _text_with_a_list_of(monkeypatch, capfd, m)
    assert t.size <= 200_000
    err0, err1 = rf._check(oracle, monkeypatch, capfd, name, t, GENERAL)
    first = _first_doubling(err0)
    assert first["a"] == m
    assert rf.BY_STATUS in err1, err1
    # the layout the comment above counts on, from the oracle's array: the list is what was asked for, place by place
    g = _list_groups(rf._oracle_sa(oracle, name, t), t, first["h"])
    assert g.size == m
    starts = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
    want = np.arange(0, m, 2) if m % 2 == 0 else np.concatenate([[0], np.arange(3, m, 2)])
    assert np.array_equal(starts, want), (m, starts[:8])
    if m % 2 and m > 2049:
        # places 2 047 and 2 048 are one group of two, cut by the end of k_group_sort's first tile of 2 048 members: no tile owns
        # it, so its two places are KEYED (k_group_sort STATUS marks what it does not own RS_PENDING | RS_KEYED, and
        # k_group_sort_straddle, which orders it, leaves RS_KEYED) -- a KEYED run from a lane's last member to the next lane's first
        assert g[2046] != g[2047] and g[2047] == g[2048] and g[2048] != g[2049]


@functools.lru_cache(maxsize=None)
def _mixed_text(seed):
    """2 000 random blocks of 8 .. 39 bytes, each copied twice: pairs everywhere in the list, and in every round those whose
    offset has run out of block split into single members -- group starts and lone members on every lane position"""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(2000):
        blk = rng.integers(1, 256, int(rng.integers(8, 40)), dtype=np.uint8)
        parts += [blk, rng.integers(1, 256, 3, dtype=np.uint8), blk, rng.integers(1, 256, 3, dtype=np.uint8)]
    return np.concatenate(parts)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_pairs_and_lone_members_mixed(oracle, monkeypatch, capfd, seed):
    t = _mixed_text(seed)
    assert t.size <= 200_000
    err0, err1 = rf._check(oracle, monkeypatch, capfd, f"helpers_mixed_{seed}", t, DENSE)
    assert _first_doubling(err0)["a"] > SPAN            # more than one workgroup of the counting kernel
    assert rf.BY_STATUS in err1, err1


@pytest.mark.gpu
@pytest.mark.parametrize("copies,pairs_shift", [(2048, rf.KEY_SYMBOLS - 2), (2048, rf.KEY_SYMBOLS - 1), (2048, rf.KEY_SYMBOLS), (4096, rf.KEY_SYMBOLS - 1)])
def test_groups_over_waves_and_tile_ends(oracle, monkeypatch, capfd, copies, pairs_shift):
    """groups of `copies` members, eight in a row, behind about 8 192 members in pairs (rf._keyed_between_owned): waves without
    any group start take their last and first start from nowhere, and the tiles' entries must still be right -- the ranks of
    the members behind them depend on it"""
    name, t = f"helpers_keyed_{copies}_{pairs_shift}", rf._keyed_between_owned(copies, pairs_shift)
    assert t.size <= 220_000
    _, err1 = rf._check(oracle, monkeypatch, capfd, name, t, DENSE)
    assert rf.BY_STATUS in err1, err1


def _flags_of_the_initial_keys(t):
    """(flags, key buffer) of the flags pass on the text's initial keys: sa_amd_test_build_keys packs them as the build does
    without gram keys, and sa_amd_test_sort_pairs_flags sorts them with the engine and the tiles of the build's initial sort"""
    t = np.ascontiguousarray(t)
    keys = np.zeros(t.size, dtype=np.uint64)
    bits, k = ctypes.c_int32(), ctypes.c_int32()
    assert sa.diag_lib().sa_amd_test_build_keys(t.ctypes.data, t.size, keys.ctypes.data, ctypes.byref(bits), ctypes.byref(k)) == 0
    # key bits as make_key_params (host/pipeline.hpp) counts them: bit fields for a power-of-two alphabet, else a base-sigma number
    sigma = max(int(np.unique(t).size), 2)
    end_bit = bits.value * k.value if bits.value else (sigma ** k.value - 1).bit_length()
    assert 0 < end_bit <= 64 and int(keys.max()).bit_length() <= end_bit, (bits.value, k.value, sigma, end_bit)
    _, flags, kout = hf._sort_flags(keys, end_bit)
    return flags, kout


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["period_8192", "english_65537", "english_1048579"])
def test_first_rerank_with_seam_flags(oracle, monkeypatch, capfd, which):
    """the first re-rank behind a flags pass, on seam texts of test_head_flags.py.  The last sort pass leaves a seam flag (two keys
    compared by the re-rank) on the first member of every digit run of each of its tiles.  In k_rr_count a seam on a lane's
    first member is bit 0 of that lane, the bit __shfl_down hands to the lane before it; a seam on a lane's last member is the
    bit whose tie depends on what the next lane hands over.  The texts must have seams on both positions, and the test fails
    if they do not.  The positions come from the flags pass itself, run on the text's initial keys; the builds without gram
    keys sort exactly those keys."""
    t = dict(hf._texts())[which]
    flags, kout = _flags_of_the_initial_keys(t)
    seam = np.flatnonzero(flags == 2)
    starts = kout[seam] != kout[seam - 1]
    for pos in (0, LANE - 1):
        here = seam % LANE == pos
        print(which, "seams on lane position", pos, ":", int(here.sum()), "of them group starts:", int((here & starts).sum()))
        assert here.any(), (which, pos, seam.size)
    exp = hf._oracle_sa(oracle, which, t)
    plain = dict(DENSE, SA_AMD_NO_GRAM_KEYS="1")
    for regime in (plain, dict(plain, SA_AMD_NO_FIRST_TAIL="1"), dict(plain, SA_AMD_BINNED_ISA_ALWAYS="1"), DENSE):
        ref, st0 = hf._build(monkeypatch, regime, t, 0)     # diagnostic library, key route
        capfd.readouterr()
        got, st1 = hf._build(monkeypatch, dict(regime, SA_AMD_VERBOSE="3"), t, 1)     # diagnostic library, flags
        assert "the last pass wrote group-start flags" in capfd.readouterr().err, regime
        prod, stp = hf._build(monkeypatch, regime, t)       # product library
        assert np.array_equal(ref, exp) and np.array_equal(got, exp) and np.array_equal(prod, exp), regime
        assert st1 == st0 and stp == st0, regime
