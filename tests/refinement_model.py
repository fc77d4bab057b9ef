"""A plain numpy model of the equivalence classes the refinement rounds are supposed to maintain, and the parser of the
per-round trace (SA_AMD_VERBOSE=3).  Nothing here touches the library: tests/test_refinement_model.py checks the model against
brute force, the oracle's suffix array and a recorded trace; tests/test_refinement_rounds.py replays the trace of real builds
through it and compares the tied counts round by round.

State is cls[i], an order-preserving dense class id per suffix, starting at 1 (the library's ranks start at 1 too).  Two
suffixes carry the same id exactly when the steps so far could not tell them apart; a smaller id means a smaller suffix.
The steps mirror what the host asks of the kernels (csrc/host/pipeline.hpp, csrc/host/refine_round.hpp), at the level of classes only:

  initial(T, k)                  the initial sort: the first k symbol codes, zero codes past the end of the text (k_build_keys)
  text_round(cls, T, depth, s)   a text-keyed round: the s padded symbols from offset depth
  rank_round(cls, h, iters)      a doubling round, dense, sparse or chasing: the classes of the suffixes i + t h, t = 1 .. iters

The number of "ranks written" that a dense round prints is NOT modelled: it depends on the tail-rank convention of the ISA
(which member of a group keeps its rank), not on the classes."""
import re

import numpy as np


def _dense(order, differs):
    """ids 1, 2, ... along `order`, a new one wherever `differs` (element r against r - 1) is set"""
    ids = np.empty(order.size, dtype=np.int64)
    ids[order] = np.cumsum(differs) if order.size else 0
    return ids


def refine(cls, *cols):
    """order-preserving dense ids of the tuples (cls[i], cols[0][i], cols[1][i], ...): one lexsort, one neighbour comparison
    per column"""
    cols = (np.asarray(cls, dtype=np.int64),) + tuple(np.asarray(c, dtype=np.int64) for c in cols)
    order = np.lexsort(cols[::-1])               # (lexsort's LAST key is the primary one)
    differs = np.ones(order.size, dtype=bool)
    if order.size:
        differs[1:] = False
        for c in cols:
            s = c[order]
            differs[1:] |= s[1:] != s[:-1]
    return _dense(order, differs)


def codes(T):
    """symbol codes: the rank of each byte value among the values that occur (code 0 = the smallest byte of the text)"""
    T = np.asarray(T, dtype=np.uint8)
    lut = np.zeros(256, dtype=np.int64)
    present = np.unique(T)
    lut[present] = np.arange(present.size)
    return lut[T]


def _window_classes(E, length):
    """order-preserving class ids of the windows E[i .. i + length) of the array E, read as zero past its end; E must end in
    a zero (then the window at the last position is the all-zero one, and every window that starts past the end equals it).
    Built by doubling: the class of a window of a + b symbols is the class of the pair (first a, following b)."""
    m = E.size
    assert m and E[-1] == 0 and length >= 1
    idx = np.arange(m)
    at = lambda c, off: c[np.minimum(idx + off, m - 1)]
    power, plen = refine(E), 1                   # classes of the windows of plen = 1, 2, 4, ... symbols
    out, olen = None, 0
    bit = 1
    while True:
        if length & bit:
            out, olen = (power, plen) if out is None else (refine(out, at(power, olen)), olen + plen)
        bit <<= 1
        if bit > length:
            return out
        power, plen = refine(power, at(power, plen)), 2 * plen


def _padded(T):
    return np.concatenate([codes(T), np.zeros(1, dtype=np.int64)])


def initial(T, k):
    """classes of the first k symbol codes of each suffix, zero codes past the end: a short suffix ties with a longer one that
    continues in the text's smallest byte"""
    n = len(T)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    return refine(_window_classes(_padded(T), int(k))[:n])


def text_round(cls, T, depth, s):
    """refine by the s padded symbols from offset depth"""
    n = len(T)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    w = _window_classes(_padded(T), int(s))
    return refine(cls, w[np.minimum(np.arange(n) + int(depth), n)])


def rank_round(cls, h, iters=1):
    """refine by the class of suffix i + t h for t = 1 .. iters, read from the classes at the start of the round.  A suffix
    whose i + t h lies past the end gets a key that is unique and smaller than every rank, the shorter suffix the smaller one:
    comp = p < n ? n + isa[p] : n - 1 - v  (text_key2<KS_RANK> and sparse_key2 in kernels/refine.hpp, chase_steps in
    kernels/lds_sort.hpp).  A chase only looks further for the members that are still tied after the steps before; for the
    classes that is the same as looking for all of them."""
    cls = np.asarray(cls, dtype=np.int64)
    n = cls.size
    i = np.arange(n, dtype=np.int64)
    cols = []
    for t in range(1, int(iters) + 1):
        p = i + t * int(h)
        inside = p < n
        cols.append(np.where(inside, n + cls[np.where(inside, p, 0)], n - 1 - i))
    return refine(cls, *cols)


def tied(cls):
    """suffixes whose class has more than one member"""
    cls = np.asarray(cls, dtype=np.int64)
    if cls.size == 0:
        return 0
    counts = np.bincount(cls)
    return int(counts[counts > 1].sum())


# ---- the trace ------------------------------------------------------------------------------------------------------------

_TEXT = re.compile(r"text round (\d+) depth (\d+): tied (\d+) -> (\d+)")
_DONE = re.compile(r"initial sort \+ text rounds \+ rank set-up done, (\d+) tied")
_DOUBLING = re.compile(r"doubling round (\d+) h (\d+) \((dense|sparse), (\d+) look-ups, (\d+) through the global sort\): "
                       r"tied (\d+) -> (\d+), (-?\d+) ranks written")


def parse_trace(stderr_text):
    """the rounds of ONE build, in the order printed: dicts with kind = "text" (round, depth, a, b), "done" (m) or "doubling"
    (round, h, mode, iters, m_global, a, b, written)"""
    out = []
    for line in stderr_text.splitlines():
        m = _TEXT.search(line)
        if m:
            r, d, a, b = map(int, m.groups())
            out.append({"kind": "text", "round": r, "depth": d, "a": a, "b": b})
            continue
        m = _DONE.search(line)
        if m:
            out.append({"kind": "done", "m": int(m.group(1))})
            continue
        m = _DOUBLING.search(line)
        if m:
            g = m.groups()
            out.append({"kind": "doubling", "round": int(g[0]), "h": int(g[1]), "mode": g[2], "iters": int(g[3]),
                        "m_global": int(g[4]), "a": int(g[5]), "b": int(g[6]), "written": int(g[7])})
    return out


def next_h(h, iters, m_global):
    """the host's rule for the next offset (doubling_rounds in csrc/host/pipeline.hpp): every group that is still tied went
    through `iters` look-ups -- unless some went through the global sort (one look-up)"""
    return h * (iters + 1 if iters > 1 and m_global == 0 else 2)
