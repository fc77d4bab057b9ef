"""Every route that works in a pooled device block (host/scope.hpp) right after a call that failed while it held a block and a
stream: sa_amd_unbwt on a (B, primary) pair that is the transform of no text answers SA_AMD_EINVAL by design, behind the ranking
phase, with everything acquired.  What it held must be back in the pool and usable: each host route and each index route
then runs once on the same text and is compared with the numpy definitions of its own test file.  The same from a second
thread, whose statistics must not show up in the first thread's.

4 097 bytes: the smallest size with more than one tile in every feature; the query of the match routes has 257 bytes."""
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from test_bwt_abi import bwt_definition, literal_cycle_length
from test_lcp import kasai
from test_lz77_abi import lpf_from_lcp, parse_definition
from test_match_abi import match_definition
from test_match_abi import spans_definition as match_spans_definition
from test_repeats_abi import keep_first_definition, repeat_lengths_definition, spans_definition

pytestmark = pytest.mark.gpu

N, M = 4097, 257
K_REPEAT, K_MATCH, CAP_MATCH = 6, 8, 64
EINVAL = -1


def moved_primary(b, primary):
    """the true transform with `primary` moved to the next valid row from which the walk closes early (numpy model)"""
    n = b.size
    for step in range(1, n):
        p = (primary - 1 + step) % n + 1
        if literal_cycle_length(b, p) != n + 1:
            return p
    raise AssertionError("every row of this transform is a valid primary")


@pytest.fixture(scope="module")
def case(oracle):
    """text, query and every expected answer, computed once and left unchanged"""
    rng = np.random.default_rng(4097)
    t = rng.integers(0, 4, N, dtype=np.uint8)
    t[2000:2200] = t[100:300]                                           # one long copy: a long phrase, long repeats
    q = np.concatenate([t[1000:1100], rng.integers(0, 256, M - 200, dtype=np.uint8), t[3000:3100]])
    assert t.size == N and q.size == M
    c = {"t": t, "q": q}
    arr = c["arr"] = oracle.sais(t)
    lcp = c["lcp"] = kasai(oracle, t, arr)
    c["bwt"] = bwt_definition(t, arr)
    c["bad_primary"] = moved_primary(*c["bwt"])
    lr = c["lr"] = repeat_lengths_definition(t, arr, lcp)
    c["spans"] = {False: spans_definition(lr, K_REPEAT)[0], True: keep_first_definition(t, arr, lcp, K_REPEAT)[0]}
    assert all(s.shape[0] > 1 for s in c["spans"].values())
    c["lpf"], c["src"] = lpf_from_lcp(t, arr, lcp)
    c["phrases"] = parse_definition(c["lpf"], c["src"])
    c["ml"], c["pos"] = match_definition(t, arr, q, CAP_MATCH)
    c["match_spans"] = match_spans_definition(t, arr, q, K_MATCH)[0]
    assert c["match_spans"].shape[0] > 1
    c["bkt"] = oracle.bucket_table(t)
    return c


def failing_call(b, primary):
    out = np.full(b.size, 0xA5, dtype=np.uint8)
    rc = sa.lib().sa_amd_unbwt(b.ctypes.data, b.size, primary, out.ctypes.data)
    assert rc == EINVAL and np.all(out == 0xA5)                         # refused, and nothing came back
    return sa.last_unbwt_stats()


def every_route(c):
    t, q, arr = c["t"], c["q"], c["arr"]
    b, p = c["bwt"]

    def eq(got, exp):
        return got.shape == exp.shape and np.array_equal(got, exp)
    # ---- host routes: the caller's array, then the array built in the block ----
    assert eq(sa.lcp(t, arr), c["lcp"])
    arr2, lcp2 = sa.saca_lcp(t)
    assert eq(arr2, arr) and eq(lcp2, c["lcp"])
    for a in (arr, None):
        b2, p2 = sa.bwt(t, a)
        assert p2 == p and eq(b2, b)
        assert eq(sa.repeat_lengths(t, a), c["lr"])
        for keep_first, exp in c["spans"].items():
            assert eq(sa.repeat_spans(t, K_REPEAT, keep_first, sa=a), exp)
        g = sa.lpf(t, a)
        assert eq(g[0], c["lpf"]) and eq(g[1], c["src"])
        assert eq(sa.lz77(t, a), c["phrases"])
    assert eq(sa.unbwt(b, p), t)
    assert eq(sa.bucket_table(t), c["bkt"])
    # ---- index routes, and the match routes (host query against the index) ----
    ix = sa.DeviceIndex(t, arr)
    try:
        assert ix.check_integrity()
        assert eq(ix.lcp(), c["lcp"])
        b2, p2 = ix.bwt()
        assert p2 == p and eq(b2, b)
        assert eq(ix.repeat_lengths(), c["lr"])
        for keep_first, exp in c["spans"].items():
            assert eq(ix.repeat_spans(K_REPEAT, keep_first), exp)
        g = ix.lpf()
        assert eq(g[0], c["lpf"]) and eq(g[1], c["src"])
        assert eq(ix.lz77(), c["phrases"])
        pats = [t[s:s + 9].tobytes() for s in range(0, N - 9, 211)] + [q[s:s + 5].tobytes() for s in range(0, M - 5, 17)]
        plain = ix.search(pats)
        for tables in (False, True):
            if tables:
                ix.enable_lcp()
            ml, pos = ix.match_stats(q, CAP_MATCH)
            assert eq(ml, c["ml"]) and eq(pos, c["pos"])
            assert eq(ix.match_spans(q, K_MATCH), c["match_spans"])
        with_lcp = ix.search(pats)
        assert sa.last_search_stats()["route"] == 1
        for key in plain:
            assert np.array_equal(plain[key], with_lcp[key]), key
    finally:
        ix.close()


def test_every_route_reuses_the_pool_after_a_failed_call(case):
    b, p = case["bwt"]
    sa.lib().sa_amd_release_cache()                                     # the failing call allocates what it hands back
    st = failing_call(b, case["bad_primary"])
    assert st["walkers"] > 0 and st["steps"] > 0                        # it got as far as the walks: block and stream were held
    every_route(case)


def test_a_failed_call_on_another_thread(case):
    t = case["t"]
    b, p = case["bwt"]
    assert np.array_equal(sa.unbwt(b, p), t)
    mine = sa.last_unbwt_stats()
    assert mine["steps"] == 2 * (N + 1)
    other = {}

    def work():
        try:
            half = b[:3001].copy()                                      # another size: other counters
            other["stats"] = failing_call(half, moved_primary(half, 1))
        except BaseException as e:      # noqa: BLE001 -- reported by the main thread
            other["error"] = repr(e)

    th = threading.Thread(target=work)
    th.start()
    th.join()
    assert "error" not in other, other
    assert other["stats"]["walkers"] > 0 and other["stats"] != mine
    assert sa.last_unbwt_stats() == mine
    every_route(case)
