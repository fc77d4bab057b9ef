"""Every refinement round of a build against the numpy model of the classes (tests/refinement_model.py).

The finished array says little about a single round: a kernel that leaves a group unsplit, a chase step that ends early or a
rank that is not written breaks the invariant the host's next offset rests on, and the array is wrong only if the skipped
symbols happen to decide an order on that text.  The number of suffixes still tied after each round is a pure function of the
text and the round's depth, and the library prints it per round (SA_AMD_VERBOSE=3).  Each build below is traced, its trace is
replayed through the model, and every count is compared with ==:

  a. tied(initial(T, k)) == last_stats()["unresolved_after_initial"] == the first count of the trace;
  b. per text round: s = this depth - the previous one (the first previous depth is k), tied(text_round(...)) == B, A == the count before;
  c. the count of the "done" line == the current count;
  d. per doubling round: the printed h == the replay's own h (the depth after the text rounds, then times I + 1 after a chase
     with nothing through the global sort, else times 2); B == tied(rank_round(cls, h, I)).  A round with I > 1 look-ups AND
     members through the global sort (one look-up) is bounded from both sides instead, tied(I look-ups) <= B <= tied(1 look-up),
     and so is every later round of that build -- no case here is expected to have one, and every case asserts that its last
     doubling round and at least one other were compared with ==;
  e. the last count is 0, and `rounds` / `text_rounds` of the statistics equal the number of lines.

Each case names the route it is there for, and the trace must show that the route was taken.  The array is compared with the
oracle as everywhere.  Model replays are cached per (text, schedule): most routes of one text share a schedule."""
import ctypes
import functools

import numpy as np
import pytest

import refinement_model as rm
import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import fibonacci_word

# ---- texts: the smallest at which each kernel structure is still reached, all above SA_AMD_SMALL_MAX ------------------------


def _blocks(seed, length, copies):
    return np.tile(np.random.default_rng(seed).integers(0, 256, length, dtype=np.uint8), copies)


def _planted():
    t = corpus.uniform(100_000, 17).copy()
    t[61_003:61_003 + 700] = t[9_001:9_001 + 700]          # 1400 tied suffixes, below n / 64
    return t


def _english_zero_tail():
    return np.concatenate([corpus.english(25_000, 23), np.zeros(5_000, dtype=np.uint8)])


def _english_zero_middle():
    e = corpus.english(25_000, 23)
    return np.concatenate([e[:12_500], np.zeros(5_000, dtype=np.uint8), e[12_500:]])


TEXTS = {
    "fibonacci": lambda: np.frombuffer(fibonacci_word(24)[:70_001], dtype=np.uint8).copy(),      # giant groups, then the chase
    "abcab": lambda: np.resize(np.frombuffer(b"abcab", dtype=np.uint8), 60_001).copy(),         # groups of n / 5 that never shrink
    "block700x97": lambda: _blocks(1, 700, 97),          # groups of 97 that straddle tiles
    "block700x130": lambda: _blocks(2, 700, 130),        # groups of 130 that straddle tiles
    "block64x4097": lambda: _blocks(3, 64, 4097),        # groups of 4097: k_group_sort_big and its upper neighbour
    "block50x8193": lambda: _blocks(4, 50, 8193),        # just above one workgroup: the global sort
    "english": lambda: corpus.english(120_000, 5),
    "dna_repeats": lambda: corpus.dna_repeats(200_000, 3),
    "uniform_planted": _planted,                          # sparse from few ties
    "english_zero_tail": _english_zero_tail,              # padding collisions at the end
    "english_zero_middle": _english_zero_middle,          # the zero run inside the text
    "twice": lambda: np.tile(corpus.english(40_000, 9), 2),
    "one_byte": lambda: np.full(20_000, 0x61, dtype=np.uint8),       # (the suite's autouse fixture keeps the closed form off)
}

# ---- routes: knobs, or a switch of the diagnostic library ------------------------------------------------------------------

_SPLIT = {"SA_AMD_SPLIT_MIN": "1", "SA_AMD_DENSE_REKEY_MIN": "1", "SA_AMD_FORCE_DENSE": "1"}      # (test_giant_groups_are_split_around_their_majority_key)
_BINNED = {"SA_AMD_BINNED_ISA_ALWAYS": "1", "SA_AMD_BINNED_MIN": "1"}

ROUTES = {
    "default": {},
    "force_dense": {"SA_AMD_FORCE_DENSE": "1"},
    "sparse_div_1": {"SA_AMD_SPARSE_DIV": "1"},
    "sparse_div_max": {"SA_AMD_SPARSE_DIV": "1000000000"},
    "sparse_div_max_1_text_round": {"SA_AMD_SPARSE_DIV": "1000000000", "SA_AMD_MAX_TEXT_ROUNDS": "1"},
    "no_text_rounds": {"SA_AMD_NO_TEXT_ROUNDS": "1"},
    "no_local_sort": {"SA_AMD_NO_LOCAL_SORT": "1"},
    "group_cap_2": {"SA_AMD_GROUP_CAP": "2"},
    "group_cap_8": {"SA_AMD_GROUP_CAP": "8"},
    "group_cap_1024": {"SA_AMD_GROUP_CAP": "1024"},
    "no_big_group_sort": {"SA_AMD_NO_BIG_GROUP_SORT": "1"},
    "network_min_0": {"SA_AMD_NETWORK_MIN": "0"},
    "network_min_1": {"SA_AMD_NETWORK_MIN": "1"},
    "chase_1": {"SA_AMD_CHASE": "1", "SA_AMD_CHASE_BIG": "1", "SA_AMD_CHASE_BIG_MIN": "1"},
    "chase_7": {"SA_AMD_CHASE": "7", "SA_AMD_CHASE_BIG": "7", "SA_AMD_CHASE_BIG_MIN": "1"},
    "binned": dict(_BINNED),
    "binned_levels_1": dict(_BINNED, SA_AMD_SCATTER_LEVELS="1"),
    "binned_levels_2": dict(_BINNED, SA_AMD_SCATTER_LEVELS="2"),
    "force_dense_binned": dict(_BINNED, SA_AMD_FORCE_DENSE="1"),
    "no_first_tail": {"SA_AMD_NO_FIRST_TAIL": "1", "SA_AMD_FORCE_DENSE": "1"},      # (the first ranks are set up on the dense route only)
    "no_defer": {"SA_AMD_NO_DEFER": "1"},
    "split_group_min_1000": dict(_SPLIT, SA_AMD_SPLIT_GROUP_MIN="1000"),
    "split_no_local": dict(_SPLIT, SA_AMD_SPLIT_GROUP_MIN="1", SA_AMD_NO_LOCAL_SORT="1"),
    "split_no_local_binned": dict(_SPLIT, SA_AMD_SPLIT_GROUP_MIN="64", SA_AMD_NO_LOCAL_SORT="1", SA_AMD_BINNED_ISA_ALWAYS="1"),
    "split_group_cap_8": dict(_SPLIT, SA_AMD_SPLIT_GROUP_MIN="1", SA_AMD_GROUP_CAP="8"),
    "no_split_no_local": dict(_SPLIT, SA_AMD_NO_SPLIT="1", SA_AMD_NO_LOCAL_SORT="1"),
    "force_top32": {"SA_AMD_FORCE_TOP32": "1"},
    "no_top32": {"SA_AMD_NO_TOP32": "1"},
    # (the bucket route and the gram keys start at 2^25 and 2^22 bytes by default: their thresholds are lowered with them)
    "top32_bucket_sort": {"SA_AMD_FORCE_TOP32": "1", "SA_AMD_BUCKET_MIN_N": "1"},
    "no_bucket_sort": {"SA_AMD_FORCE_TOP32": "1", "SA_AMD_BUCKET_MIN_N": "1", "SA_AMD_NO_BUCKET_SORT": "1"},
    "gram_keys": {"SA_AMD_GRAM_MIN_N": "1"},
    "no_gram_keys": {"SA_AMD_GRAM_MIN_N": "1", "SA_AMD_NO_GRAM_KEYS": "1"},
    "gram_3": {"SA_AMD_GRAM_G": "3", "SA_AMD_GRAM_MIN_N": "1"},
    "no_fused_finish": {"SA_AMD_NO_FUSED_FINISH": "1", "SA_AMD_FORCE_TOP32": "1"},
    "fused64": {"SA_AMD_FUSED64": "1"},
    # the diagnostic library (built from the same sources), as tests/test_head_flags.py and tests/test_rerank_routes.py load it
    "head_flags_0": ({"SA_AMD_FORCE_DENSE": "1"}, "sa_amd_debug_head_flags", 0),
    "head_flags_2": ({}, "sa_amd_debug_head_flags", 2),
    "rerank_routes_1": ({"SA_AMD_FORCE_DENSE": "1"}, "sa_amd_debug_rerank_routes", 1),
    "rerank_routes_2": ({"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"}, "sa_amd_debug_rerank_routes", 2),
    "rerank_routes_3": ({"SA_AMD_FORCE_DENSE": "1", "SA_AMD_BINNED_ISA_ALWAYS": "1"}, "sa_amd_debug_rerank_routes", 3),
}


def _route(route):
    r = ROUTES[route]
    return (r, None, None) if isinstance(r, dict) else r


def traced_build(monkeypatch, capture, t, route):
    """(array, statistics, stderr of the build) -- capture.readouterr() is pytest's capfd (the library's fprintf(stderr) is
    unbuffered and the knob is read per build)"""
    env, switch, value = _route(route)
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        m.setenv("SA_AMD_VERBOSE", "3")
        capture.readouterr()
        if switch is None:
            out, st = sa.SuffixArray(t).into_parts()[1], sa.last_stats()
        else:
            L = sa.diag_lib()
            fn = getattr(L, switch)
            fn.argtypes, fn.restype = [ctypes.c_int32], ctypes.c_int32
            L.sa_amd_saca_u8.argtypes, L.sa_amd_saca_u8.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32], ctypes.c_int32
            t = np.ascontiguousarray(t)
            out = np.zeros(t.size + 1, dtype=np.uint32)
            stats = sa.Stats()
            before = fn(value)
            try:
                assert L.sa_amd_saca_u8(t.ctypes.data, out.ctypes.data, t.size) == 0
            finally:
                fn(before if switch == "sa_amd_debug_head_flags" else 0)
            L.sa_amd_last_stats(ctypes.addressof(stats))
            st = stats.as_dict()
        err = capture.readouterr().err
    return out, st, err


# ---- the replay -----------------------------------------------------------------------------------------------------------

class Model:
    """the model's tied counts along schedules of one text, cached: a schedule is a tuple of steps ("initial", k),
    ("text", depth, s), ("rank", h, fine look-ups, coarse look-ups).  A count is a pair (fine, coarse); the two differ only
    behind a round that is bounded from both sides.  Class vectors are kept along the latest schedule only."""

    def __init__(self, t):
        self.t = t
        self.counts = {}
        self.states = {}

    def _apply(self, state, step):
        fine, coarse = state
        if step[0] == "initial":
            fine = coarse = rm.initial(self.t, step[1])
        elif step[0] == "text":
            same = fine is coarse
            fine = rm.text_round(fine, self.t, step[1], step[2])
            coarse = fine if same else rm.text_round(coarse, self.t, step[1], step[2])
        else:
            _, h, i_fine, i_coarse = step
            same = fine is coarse and i_fine == i_coarse
            fine, coarse = rm.rank_round(fine, h, i_fine), (None if same else rm.rank_round(coarse, h, i_coarse))
            if same:
                coarse = fine
        return fine, coarse

    def _state(self, steps):
        if not steps:
            return None, None
        if steps not in self.states:
            new = self._apply(self._state(steps[:-1]), steps[-1])
            self.states = {k: v for k, v in self.states.items() if k == steps[:len(k)]}      # (the latest path only)
            self.states[steps] = new
            self.counts[steps] = (rm.tied(new[0]), rm.tied(new[1]))
        return self.states[steps]

    def tied(self, steps):
        if steps not in self.counts:
            self._state(steps)
        return self.counts[steps]


def replay(model, stats, rounds):
    """checks a - e; returns (rounds compared with ==, rounds bounded from both sides, the last doubling round was compared with ==)"""
    k = stats["symbols_per_key"]
    steps = (("initial", k),)
    now = model.tied(steps)
    assert now[0] == now[1] == stats["unresolved_after_initial"], ("a", now, stats)
    first = next((r["m"] if r["kind"] == "done" else r["a"]) for r in rounds)
    assert first == now[0], ("a: the first count of the trace", first, now)
    depth, h, exact, bounded, last_exact = k, None, 0, 0, False
    between = False                       # behind a round that was bounded from both sides: so is every later one
    kinds = [r["kind"] for r in rounds]
    assert kinds.count("done") == 1 and kinds == ["text"] * kinds.index("done") + ["done"] + ["doubling"] * (len(kinds) - kinds.index("done") - 1), kinds
    number = 0
    for r in rounds:
        if r["kind"] == "text":
            number += 1
            assert r["round"] == number and r["depth"] > depth, ("b", r)
            assert r["a"] == now[0] == now[1], ("b: A", r, now)
            steps += (("text", depth, r["depth"] - depth),)
            depth = r["depth"]
            now = model.tied(steps)
            assert r["b"] == now[0], ("b: B", r, now)
            exact += 1
        elif r["kind"] == "done":
            assert r["m"] == now[0] == now[1], ("c", r, now)
            h = depth
        else:
            number += 1
            assert r["round"] == number, ("d", r)
            assert r["h"] == h, ("d: h", r, h)
            if not between:
                assert r["a"] == now[0] == now[1], ("d: A", r, now)
            sandwich = r["iters"] > 1 and r["m_global"] > 0
            between = between or sandwich
            steps += (("rank", h, r["iters"], 1 if sandwich else r["iters"]),)
            now = model.tied(steps)
            if not between:
                assert r["b"] == now[0] == now[1], ("d: B", r, now)
                exact += 1
                last_exact = True
            else:
                assert now[0] <= r["b"] <= now[1], ("d: B between", r, now)
                bounded += 1
                last_exact = False
            h = rm.next_h(h, r["iters"], r["m_global"])
    last = rounds[-1]
    assert (last["m"] if last["kind"] == "done" else last["b"]) == 0, ("e", last)
    assert stats["rounds"] == number and stats["text_rounds"] == kinds.count("text"), ("e", stats, kinds)
    return exact, bounded, last_exact


def route_taken(name, stats, rounds):
    doubling = [r for r in rounds if r["kind"] == "doubling"]
    if name == "chase":
        return any(r["iters"] > 1 and r["m_global"] == 0 for r in doubling)
    if name == "global":
        return any(r["m_global"] > 0 for r in doubling)
    if name == "local only":
        return bool(doubling) and all(r["m_global"] == 0 for r in doubling)
    if name == "text":
        return stats["text_rounds"] >= 1
    if name == "sparse":
        return any(r["mode"] == "sparse" for r in doubling) and stats["sparse_mode"] == 1
    if name == "dense":
        return any(r["mode"] == "dense" for r in doubling)
    if name == "top32":
        return stats["top32_first"] == 1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def text_of(name):
    t = TEXTS[name]()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def model_of(name):
    return Model(text_of(name))


_expected = {}


def expected_array(oracle, name):
    if name not in _expected:
        _expected[name] = oracle.sais(text_of(name))
    return _expected[name]


# (text, route, what the case is there for: the trace must show it)
CASES = [
    ("fibonacci", "default", ('chase', 'local only', 'text', 'dense')),
    ("abcab", "default", ('global', 'text', 'dense')),
    ("block700x97", "default", ('chase', 'local only', 'text', 'dense')),
    ("block700x130", "default", ('chase', 'local only', 'text', 'dense')),
    ("block64x4097", "default", ('global', 'text', 'dense')),
    ("block50x8193", "default", ('global', 'text', 'dense')),
    ("english", "default", ('local only', 'text', 'sparse')),
    ("dna_repeats", "default", ('chase', 'local only', 'text', 'dense')),
    ("uniform_planted", "default", ('local only', 'sparse')),
    ("english_zero_tail", "default", ('global', 'text', 'dense')),
    ("english_zero_middle", "default", ('global', 'text', 'dense')),
    ("twice", "default", ('chase', 'local only', 'text', 'dense')),
    ("one_byte", "default", ('global', 'text', 'dense')),
    ("fibonacci", "force_dense", ('chase', 'global', 'dense')),
    ("block700x97", "force_dense", ('chase', 'local only', 'dense')),
    ("block64x4097", "force_dense", ('global', 'dense')),
    ("dna_repeats", "force_dense", ('chase', 'local only', 'dense')),
    ("english_zero_tail", "force_dense", ('global', 'dense')),
    ("twice", "force_dense", ('chase', 'local only', 'dense')),
    ("fibonacci", "sparse_div_1", ('global', 'sparse')),
    ("block700x130", "sparse_div_1", ('local only', 'sparse')),
    ("block64x4097", "sparse_div_1", ('global', 'sparse')),
    ("uniform_planted", "sparse_div_1", ('local only', 'sparse')),
    ("english_zero_middle", "sparse_div_1", ('global', 'sparse')),
    ("twice", "sparse_div_1", ('local only', 'sparse')),
    ("one_byte", "sparse_div_1", ('global', 'sparse')),
    ("dna_repeats", "sparse_div_max", ('chase', 'local only', 'text', 'dense')),
    ("twice", "sparse_div_max", ('chase', 'local only', 'text', 'dense')),
    ("uniform_planted", "sparse_div_max", ('chase', 'local only', 'text', 'dense')),
    ("english", "sparse_div_max_1_text_round", ('local only', 'text', 'dense')),
    ("fibonacci", "sparse_div_max_1_text_round", ('chase', 'local only', 'text', 'dense')),
    ("english_zero_tail", "sparse_div_max_1_text_round", ('global', 'text', 'dense')),
    ("fibonacci", "no_text_rounds", ('chase', 'global', 'dense')),
    ("abcab", "no_text_rounds", ('global', 'dense')),
    ("twice", "no_text_rounds", ('chase', 'local only', 'dense')),
    ("fibonacci", "no_local_sort", ('global', 'text', 'dense')),
    ("block700x97", "no_local_sort", ('global', 'text', 'dense')),
    ("dna_repeats", "no_local_sort", ('global', 'text', 'dense')),
    ("twice", "no_local_sort", ('global', 'text', 'dense')),
    ("uniform_planted", "no_local_sort", ('global', 'sparse')),
    ("fibonacci", "group_cap_2", ('global', 'text', 'dense')),
    ("block700x97", "group_cap_2", ('global', 'text', 'dense')),
    ("dna_repeats", "group_cap_2", ('chase', 'global', 'text', 'dense')),
    ("fibonacci", "group_cap_8", ('chase', 'global', 'text', 'dense')),
    ("block700x130", "group_cap_8", ('global', 'text', 'dense')),
    ("twice", "group_cap_8", ('chase', 'local only', 'text', 'dense')),
    ("block700x130", "group_cap_1024", ('chase', 'local only', 'text', 'dense')),
    ("block64x4097", "group_cap_1024", ('global', 'text', 'dense')),
    ("fibonacci", "no_big_group_sort", ('chase', 'local only', 'text', 'dense')),
    ("block64x4097", "no_big_group_sort", ('global', 'text', 'dense')),
    ("block50x8193", "no_big_group_sort", ('global', 'text', 'dense')),
    ("fibonacci", "network_min_0", ('chase', 'local only', 'text', 'dense')),
    ("block700x130", "network_min_0", ('chase', 'local only', 'text', 'dense')),
    ("twice", "network_min_0", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "network_min_1", ('chase', 'local only', 'text', 'dense')),
    ("block700x97", "network_min_1", ('chase', 'local only', 'text', 'dense')),
    ("twice", "network_min_1", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "chase_1", ('local only', 'text', 'dense')),
    ("block700x97", "chase_1", ('local only', 'text', 'dense')),
    ("twice", "chase_1", ('local only', 'text', 'dense')),
    ("fibonacci", "chase_7", ('chase', 'local only', 'text', 'dense')),
    ("block700x130", "chase_7", ('chase', 'local only', 'text', 'dense')),
    ("dna_repeats", "chase_7", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "binned", ('chase', 'local only', 'text', 'dense')),
    ("abcab", "binned", ('global', 'text', 'dense')),
    ("twice", "binned", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "binned_levels_1", ('chase', 'local only', 'text', 'dense')),
    ("twice", "binned_levels_1", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "binned_levels_2", ('chase', 'local only', 'text', 'dense')),
    ("block50x8193", "binned_levels_2", ('global', 'text', 'dense')),
    ("fibonacci", "force_dense_binned", ('chase', 'global', 'dense')),
    ("twice", "force_dense_binned", ('chase', 'local only', 'dense')),
    ("english_zero_middle", "force_dense_binned", ('global', 'dense')),
    ("fibonacci", "no_first_tail", ('chase', 'global', 'dense')),
    ("block700x97", "no_first_tail", ('chase', 'local only', 'dense')),
    ("twice", "no_first_tail", ('chase', 'local only', 'dense')),
    ("one_byte", "no_first_tail", ('global', 'dense')),
    ("fibonacci", "no_defer", ('chase', 'local only', 'text', 'dense')),
    ("twice", "no_defer", ('chase', 'local only', 'text', 'dense')),
    ("english", "no_defer", ('local only', 'text', 'sparse')),
    ("block700x130", "no_defer", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "split_group_min_1000", ('chase', 'global', 'dense')),
    ("abcab", "split_group_min_1000", ('global', 'dense')),
    ("one_byte", "split_group_min_1000", ('global', 'dense')),
    ("fibonacci", "split_no_local", ('global', 'dense')),
    ("abcab", "split_no_local", ('global', 'dense')),
    ("block50x8193", "split_no_local", ('global', 'dense')),
    ("fibonacci", "split_no_local_binned", ('global', 'dense')),
    ("one_byte", "split_no_local_binned", ('global', 'dense')),
    ("fibonacci", "split_group_cap_8", ('chase', 'global', 'dense')),
    ("abcab", "split_group_cap_8", ('global', 'dense')),
    ("block700x97", "split_group_cap_8", ('global', 'dense')),
    ("fibonacci", "no_split_no_local", ('global', 'dense')),
    ("abcab", "no_split_no_local", ('global', 'dense')),
    ("english", "force_top32", ('local only', 'text', 'sparse', 'top32')),
    ("twice", "force_top32", ('chase', 'local only', 'text', 'dense', 'top32')),
    ("uniform_planted", "force_top32", ('local only', 'sparse', 'top32')),
    ("english_zero_tail", "force_top32", ('global', 'text', 'dense', 'top32')),
    ("english", "no_top32", ('local only', 'text', 'sparse')),
    ("twice", "no_top32", ('chase', 'local only', 'text', 'dense')),
    ("english", "top32_bucket_sort", ('local only', 'text', 'sparse', 'top32')),
    ("dna_repeats", "top32_bucket_sort", ('chase', 'local only', 'text', 'dense', 'top32')),
    ("uniform_planted", "top32_bucket_sort", ('local only', 'sparse', 'top32')),
    ("english", "no_bucket_sort", ('local only', 'text', 'sparse', 'top32')),
    ("dna_repeats", "no_bucket_sort", ('chase', 'local only', 'text', 'dense', 'top32')),
    ("twice", "gram_keys", ('chase', 'local only', 'text', 'dense')),
    ("block50x8193", "gram_keys", ('global', 'text', 'dense')),
    ("dna_repeats", "gram_keys", ('chase', 'local only', 'text', 'dense')),
    ("english_zero_tail", "gram_keys", ('global', 'text', 'dense')),
    ("twice", "no_gram_keys", ('chase', 'local only', 'text', 'dense')),
    ("dna_repeats", "no_gram_keys", ('chase', 'local only', 'text', 'dense')),
    ("twice", "gram_3", ('chase', 'local only', 'text', 'dense')),
    ("block64x4097", "gram_3", ('global', 'text', 'dense')),
    ("uniform_planted", "gram_3", ('local only', 'sparse')),
    ("english_zero_middle", "gram_3", ('global', 'text', 'dense')),
    ("english", "no_fused_finish", ('local only', 'text', 'sparse', 'top32')),
    ("twice", "no_fused_finish", ('chase', 'local only', 'text', 'dense', 'top32')),
    ("dna_repeats", "no_fused_finish", ('chase', 'local only', 'text', 'dense', 'top32')),
    ("fibonacci", "fused64", ('chase', 'local only', 'text', 'dense')),
    ("twice", "fused64", ('chase', 'local only', 'text', 'dense')),
    ("dna_repeats", "fused64", ('chase', 'local only', 'text', 'dense')),
    ("english", "fused64", ('local only', 'text', 'sparse')),
    ("one_byte", "fused64", ('global', 'text', 'dense')),
    ("block700x130", "fused64", ('chase', 'local only', 'text', 'dense')),
    ("fibonacci", "head_flags_0", ('chase', 'global', 'dense')),
    ("twice", "head_flags_0", ('chase', 'local only', 'dense')),
    ("block700x97", "head_flags_0", ('chase', 'local only', 'dense')),
    ("fibonacci", "head_flags_2", ('chase', 'local only', 'text', 'dense')),
    ("twice", "head_flags_2", ('chase', 'local only', 'text', 'dense')),
    ("english", "head_flags_2", ('local only', 'text', 'sparse')),
    ("fibonacci", "rerank_routes_1", ('chase', 'global', 'dense')),
    ("twice", "rerank_routes_1", ('chase', 'local only', 'dense')),
    ("abcab", "rerank_routes_1", ('global', 'dense')),
    ("fibonacci", "rerank_routes_2", ('chase', 'global', 'dense')),
    ("twice", "rerank_routes_2", ('chase', 'local only', 'dense')),
    ("block700x130", "rerank_routes_2", ('chase', 'local only', 'dense')),
    ("fibonacci", "rerank_routes_3", ('chase', 'global', 'dense')),
    ("twice", "rerank_routes_3", ('chase', 'local only', 'dense')),
    ("one_byte", "rerank_routes_3", ('global', 'dense')),
]


@pytest.mark.gpu
@pytest.mark.parametrize("text,route,wanted", CASES, ids=[f"{t}-{r}" for t, r, _ in CASES])
def test_every_round_leaves_the_models_tied_count(oracle, monkeypatch, capfd, text, route, wanted):
    t = text_of(text)
    assert t.size > 8192                        # above SA_AMD_SMALL_MAX: the staged pipeline runs
    got, stats, err = traced_build(monkeypatch, capfd, t, route)
    assert np.array_equal(got, expected_array(oracle, text))
    rounds = rm.parse_trace(err)
    for name in wanted:
        assert route_taken(name, stats, rounds), (name, stats, rounds)
    exact, bounded, last_exact = replay(model_of(text), stats, rounds)
    print(f"{text} {route}: {exact} rounds compared with ==, {bounded} bounded from both sides")
    assert last_exact and exact >= 2, (exact, bounded, rounds)
    assert bounded == 0 or any(r["iters"] > 1 and r["m_global"] > 0 for r in rounds if r["kind"] == "doubling")
