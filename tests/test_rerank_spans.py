"""The counting kernels of the re-rank cover a SPAN of tiles per workgroup where a member is one byte (k_rr_count<..., FLAGS>,
kernels/rerank.hpp; k_flag_count<STATUS>, kernels/refine.hpp): RR_COUNT_SPAN = 4 tiles of 8 192 members, S = 32 768 members.
A workgroup issues the byte loads of the whole span first, classifies tile by tile, and its waves 0 .. 3 write one
tile_cnt / tile_head / tile_first entry each -- tile_head through ONE look-up of the slot of the tile's last group start.

What can go wrong there, and the smallest texts at which it would:
  * a list that ends inside the last tile of a span, exactly on a span, one member into the next span (a workgroup whose later
    tiles do not exist must write nothing for them and still count the tile the list ends in);
  * places whose keys are read (RS_KEYED) in runs that start on a wave start, mid-wave and on a tile start, in the second,
    third and fourth tile of a span;
  * the first re-rank behind a flags pass (the flag form of the same kernel).
The kernel does not loop over spans (the grid is the number of spans), so there is no capped-grid case.  The wave-striped key
read for KEYED runs was measured and not kept (CHANGELOG), so there is no threshold to put texts around; the KEYED family stays:
it is the per-lane key read inside a span, behind byte loads that were issued tiles earlier.

Every build is the oracle's array; statistics and per-round tied counts are those of the key route of the diagnostic library
(sa_amd_debug_round_flags(0) / sa_amd_debug_head_flags(0)), as in test_round_flags.py and test_head_flags.py, whose generators
and build helpers are used here."""
import numpy as np
import pytest

from suffix_array_amd import corpus
import refinement_model as rm
import test_head_flags as hf
import test_round_flags as rf

RR_TILE = 8192
S = 4 * RR_TILE          # members one workgroup of k_rr_count<..., FLAGS> covers (RR_COUNT_SPAN tiles)
DENSE = {"SA_AMD_FORCE_DENSE": "1"}

LIST_LENGTHS = [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 8191, 8192, 8193]


def _first_doubling(err):
    return [r for r in rm.parse_trace(err) if r["kind"] == "doubling"][0]


def _list_length_text(m, k, salt):
    """rf._list_length_text for a key of k symbols: random bytes, one block of m // 2 + k - 1 bytes copied twice (a pair of tied
    suffixes for every offset that leaves k bytes of the block) and, for an odd m, one block of k bytes copied three times"""
    pairs = (m - 3) // 2 if m % 2 else m // 2
    seed = 100_000 * salt + m
    B, C = rf._rnd(7000 + seed, pairs + k - 1), rf._rnd(8000 + seed, k)
    parts = [rf._rnd(9000 + seed, 3000), B, rf._rnd(9001 + seed, 1500), B, rf._rnd(9002 + seed, 2500)]
    if m % 2:
        parts += [C, rf._rnd(9003 + seed, 700), C, rf._rnd(9004 + seed, 900), C, rf._rnd(9005 + seed, 1100)]
    return np.concatenate(parts)


def _text_with_a_list_of(monkeypatch, capfd, m):
    """The key of the initial sort holds fewer symbols on longer texts (5 at the longer ones here, 8 at the lengths of
    test_round_flags.py), and two unrelated suffixes of the text may share a key of 5 random bytes (about one text in a thousand): the first doubling round of a
    key-route build says how many symbols the key held and how long the list is, and the text is made again until both fit."""
    k = rf.KEY_SYMBOLS
    for salt in range(6):
        t = _list_length_text(m, k, salt)
        first = _first_doubling(rf._build(monkeypatch, capfd, DENSE, t, 0)[2])
        if first["h"] == k and first["a"] == m:
            return t
        k = first["h"]
    raise AssertionError((m, first))


@pytest.mark.gpu
@pytest.mark.parametrize("m", LIST_LENGTHS)
def test_list_ends_around_a_span(oracle, monkeypatch, capfd, m):
    name, t = f"span_list_of_{m}", _text_with_a_list_of(monkeypatch, capfd, m)
    assert t.size <= 100_000
    err0, err1 = rf._check(oracle, monkeypatch, capfd, name, t, DENSE)
    assert _first_doubling(err0)["a"] == m             # the list the first doubling round re-ranks has the length asked for
    assert rf.BY_STATUS in err1, err1                  # ... and that round read status bytes


@pytest.mark.gpu
@pytest.mark.parametrize("big_groups", ["in_lds", "global_sort"])
@pytest.mark.parametrize("pairs_shift", [rf.KEY_SYMBOLS - 2, rf.KEY_SYMBOLS - 1, rf.KEY_SYMBOLS])
@pytest.mark.parametrize("copies", [2048, 8192, 16384])
def test_keyed_runs_inside_a_span(oracle, monkeypatch, capfd, copies, pairs_shift, big_groups):
    """runs of `copies` KEYED places each, eight of them in a row, behind about 8 192 owned members: with the three shifts the
    first run starts mid-wave, on a wave start and on a tile start, and the runs reach through the tiles of the first spans"""
    env = dict(DENSE) if big_groups == "in_lds" else dict(DENSE, SA_AMD_NO_BIG_GROUP_SORT="1")
    name, t = f"span_keyed_{copies}_{pairs_shift}", rf._keyed_between_owned(copies, pairs_shift)
    _, err1 = rf._check(oracle, monkeypatch, capfd, name, t, env)
    assert rf.BY_STATUS in err1, err1


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8193, 65537])
def test_first_rerank_behind_a_flags_pass(oracle, monkeypatch, n):
    name, t = f"span_english_{n}", corpus.english(n, 5)
    exp = hf._oracle_sa(oracle, name, t)
    ref, st0 = hf._build(monkeypatch, DENSE, t, 0)     # diagnostic library, key route
    got, st1 = hf._build(monkeypatch, DENSE, t, 1)     # diagnostic library, flags
    prod, stp = hf._build(monkeypatch, DENSE, t)       # product library
    assert np.array_equal(ref, exp) and np.array_equal(got, exp) and np.array_equal(prod, exp)
    assert st1 == st0 and stp == st0
