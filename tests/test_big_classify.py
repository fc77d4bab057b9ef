"""k_big_classify (kernels/refine.hpp): the heads that k_group_sort lists for k_group_sort_big are sorted once into one list per
instance -- groups of GS_CAP + 1 .. GB_CAP_SMALL members, groups of GB_CAP_SMALL + 1 .. GB_CAP members -- and each instance walks
its own list.  A head of neither class goes nowhere: its group is k_group_sort_straddle's or the global sort's.

The texts follow the keyed family of tests/test_round_flags.py: a 24-byte block repeated `size` times gives groups of exactly `size`
members in the first doubling round, padding in front of them (pairs of tied suffixes over smaller byte values) puts the first
member of the first such group on a chosen place of a 2 048-member k_group_sort tile.  The place is not assumed: a numpy model of
the initial classes (tests/refinement_model.py) and the oracle's array give the tied list of the first round, and the test
asserts that a group of the wanted size starts on the wanted place.

Every text is built with and without SA_AMD_NO_BIG_GROUP_SORT=1: the array is the oracle's both times, the rounds and their tied
counts are the same, and the members that the local pass ordered beyond those of the build without k_group_sort_big are at least
the groups of the first round that the model says are k_group_sort_big's."""
import functools

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
import refinement_model as rm

GS_TILE, GS_CAP, GB_CAP_SMALL, GB_CAP, GB_LIST_MIN = 2048, 1024, 4096, 8192, 256      # kernels/refine.hpp
# SA_AMD_CHASE=1: one look-up per member and round, so that both builds of a text take the same rounds
ENV = {"SA_AMD_FORCE_DENSE": "1", "SA_AMD_NO_GRAM_KEYS": "1", "SA_AMD_CHASE": "1"}
SIZES = (1024, 1025, 4096, 4097, 8192, 8193)
# first member of the group: first place of a tile, in its middle, and across its end with exactly GB_LIST_MIN members inside the
# tile (listed) and with one fewer (not listed: the global sort's, whatever its size)
PLACES = (0, 1000, GS_TILE - GB_LIST_MIN, GS_TILE - GB_LIST_MIN + 1)


def _rnd(seed, count, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi, count, dtype=np.uint8)


def _text(size, pairs, triple):
    """pairs + 7 bytes below 0x10 copied twice (a pair of tied suffixes per offset that leaves a whole key) and, for an odd number
    of members in front, 8 such bytes copied three times; the block repeated `size` times; untied bytes; every byte value once"""
    filler = lambda s, c: _rnd(s, c, 0x70, 0xF0)
    small = _rnd(31 + size, pairs + 7, 0, 0x10)
    parts = [small, filler(1, 40), small, filler(2, 40)]
    if triple:
        c = _rnd(57 + size, 8, 0, 0x10)
        parts += [c, filler(3, 40), c, filler(4, 40), c, filler(5, 40)]
    block = np.concatenate([_rnd(200 + size, 8, 0x10, 0x60), np.arange(0x60, 0x70, dtype=np.uint8)])
    parts += [np.tile(block, size), filler(6, 12 * size), np.arange(256, dtype=np.uint8)]
    return np.concatenate(parts)


def _first_round_groups(t, k, exp):
    """(list position of the first member, members) of every group of the tied list behind an initial sort on k symbols"""
    cls = rm.initial(t, k)
    c = cls[exp[1:].astype(np.int64)]
    lc = c[np.bincount(cls)[c] > 1]
    starts = np.flatnonzero(np.concatenate([[True], lc[1:] != lc[:-1]]))
    return starts, np.diff(np.concatenate([starts, [lc.size]]))


def _big_members(starts, sizes):
    """members of the groups that k_group_sort lists and k_big_classify hands to one of the two instances"""
    at = starts % GS_TILE
    listed = np.where(at + sizes <= GS_TILE, sizes > GS_CAP, GS_TILE - at >= GB_LIST_MIN)
    return int(sizes[listed & (sizes > GS_CAP) & (sizes <= GB_CAP)].sum())


def _build(monkeypatch, capfd, t, extra):
    with monkeypatch.context() as m:
        for k, v in dict(ENV, **extra).items():
            m.setenv(k, v)
        m.setenv("SA_AMD_VERBOSE", "3")
        capfd.readouterr()
        out, st = sa.SuffixArray(t).into_parts()[1], sa.last_stats()
        rounds = [(r["kind"], r.get("a", r.get("m")), r.get("b"), r.get("h")) for r in rm.parse_trace(capfd.readouterr().err)]
    return out, st, rounds


def _check(oracle, monkeypatch, capfd, t, exp):
    """both builds of a text; returns (statistics with k_group_sort_big, members only it let the local pass order)"""
    got, st, rounds = _build(monkeypatch, capfd, t, {})
    assert np.array_equal(got, exp)
    got0, st0, rounds0 = _build(monkeypatch, capfd, t, {"SA_AMD_NO_BIG_GROUP_SORT": "1"})
    assert np.array_equal(got0, exp)
    assert rounds == rounds0 and st["rounds"] == st0["rounds"] and len(rounds) > 1, (rounds, rounds0)
    for key in ("symbols_per_key", "unresolved_after_initial", "text_rounds", "sparse_mode"):
        assert st[key] == st0[key], (key, st, st0)
    return st, st["locally_sorted"] - st0["locally_sorted"]


@functools.lru_cache(maxsize=None)
def _key_symbols():
    """symbols per key of the texts below (every byte value occurs, plain keys: 8), from a build"""
    with pytest.MonkeyPatch.context() as m:
        for k, v in ENV.items():
            m.setenv(k, v)
        sa.SuffixArray(_text(1025, 8, False)).into_parts()
        return sa.last_stats()["symbols_per_key"]


@pytest.mark.gpu
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("size", SIZES)
def test_group_of_every_class_on_every_place(oracle, monkeypatch, capfd, size, place):
    k = _key_symbols()
    # the members in front of the block's groups: 2 per pair, 3 for the triple
    triple = place % 2 == 1
    base = _text(size, 8, triple)
    starts, sizes = _first_round_groups(base, k, oracle.sais(base))
    first = int(starts[np.flatnonzero(sizes == size)[0]])
    assert (place - first) % 2 == 0, (first, place)
    t = _text(size, 8 + ((place - first) % GS_TILE) // 2, triple)
    exp = oracle.sais(t)
    starts, sizes = _first_round_groups(t, k, exp)
    hit = (sizes == size) & (starts % GS_TILE == place)
    assert hit.any(), (size, place, starts[sizes == size] % GS_TILE)
    st, gained = _check(oracle, monkeypatch, capfd, t, exp)
    assert st["symbols_per_key"] == k
    want = _big_members(starts, sizes)
    print(f"size {size} place {place}: first round has {want} members for k_group_sort_big, it ordered {gained} in all rounds")
    if GS_CAP < size <= GB_CAP and place <= GS_TILE - GB_LIST_MIN:
        assert want >= size                      # (the group made for this case is among them)
    assert gained >= want, (gained, want)


@pytest.mark.gpu
def test_no_listed_head(oracle, monkeypatch, capfd):
    """many small groups and none of more than GB_LIST_MIN members: k_group_sort lists nothing, all three launches see a count of 0"""
    t = corpus.english(150_000, 9)
    exp = oracle.sais(t)
    _, sizes = _first_round_groups(t, _english_key_symbols(), exp)
    assert sizes.size > 1000 and sizes.max() < GB_LIST_MIN, sizes.max()
    _, gained = _check(oracle, monkeypatch, capfd, t, exp)
    assert gained == 0


@functools.lru_cache(maxsize=None)
def _english_key_symbols():
    with pytest.MonkeyPatch.context() as m:
        for k, v in ENV.items():
            m.setenv(k, v)
        sa.SuffixArray(corpus.english(150_000, 9)).into_parts()
        return sa.last_stats()["symbols_per_key"]


@pytest.mark.gpu
def test_every_head_belongs_to_the_global_sort(oracle, monkeypatch, capfd):
    """a block repeated 20 000 times: the groups lose one member a round and stay above GB_CAP until the periods are told apart, so
    every listed head is classified into neither list and k_group_sort_big orders nothing"""
    block = np.concatenate([_rnd(77, 8, 0x10, 0x60), np.arange(0x60, 0x70, dtype=np.uint8)])
    t = np.concatenate([np.tile(block, 20_000), _rnd(78, 500_000, 0x70, 0xF0), np.arange(256, dtype=np.uint8)])
    exp = oracle.sais(t)
    starts, sizes = _first_round_groups(t, _key_symbols(), exp)
    assert sizes.size == 24 and sizes.min() > GB_CAP and _big_members(starts, sizes) == 0
    _, gained = _check(oracle, monkeypatch, capfd, t, exp)
    assert gained == 0
