"""CPU suite for the LCP-accelerated search of the device index (kernels/esa.hpp): the exports, the
argument check that answers without a device, and the algorithm restated in numpy -- the pair table of the aligned search
tree and the two Manber-Myers descents -- against oracle/search_model.py, with and without the bucket table, together with
the bound on the text bytes compared."""
import ctypes
import zlib

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import adversarial_cases, fibonacci_word

import search_model

EXPORTS = ("sa_amd_index_enable_lcp", "sa_amd_last_search_stats")
WAVE = 64


def test_library_exports_the_lcp_search_entry_points():
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert hasattr(L, fn), fn
    assert callable(sa.last_search_stats)
    assert callable(sa.DeviceIndex.enable_lcp) and callable(sa.SuffixArray.enable_lcp)
    assert ctypes.sizeof(sa.SearchStats) == 40


def test_enable_lcp_of_null_index_is_einval():
    assert sa.lib().sa_amd_index_enable_lcp(None) == -1


# ---- the model ----

def kasai(t, arr):
    n = len(t)
    lcp = np.zeros(n + 1, dtype=np.int64)
    rank = np.empty(n + 1, dtype=np.int64)
    rank[np.asarray(arr, dtype=np.int64)] = np.arange(n + 1)
    h = 0
    for p in range(n):
        r = rank[p]
        q = int(arr[r - 1])
        while p + h < n and q + h < n and t[p + h] == t[q + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return lcp


def log_p(n):
    k = 1
    while (1 << k) < n + 2:
        k += 1
    return k


def pair_table(lcp):
    """pair[x - 1] = (Llcp, Rlcp) of node x = 1 .. N: the minima of the two halves of x's aligned block of 2 lowbit(x)"""
    N = lcp.size
    P = 1 << log_p(N - 1)
    B = np.zeros(P, dtype=np.int64)
    B[:N] = lcp
    pair = np.full((N, 2), -1, dtype=np.int64)
    mins = B
    h = 1
    while h < P:
        x = np.arange(h, P, 2 * h)                     # nodes of this level: odd multiples of h
        real = x <= N
        pair[x[real] - 1, 0] = mins[0::2][real]
        pair[x[real] - 1, 1] = mins[1::2][real]
        mins = np.minimum(mins[0::2], mins[1::2])
        h *= 2
    assert (pair >= 0).all()
    return pair


def compare_from(t, p, pat, c0, cnt):
    """wave_compare_from: ord of t[p:] against pat and their lcp, knowing the first c0 bytes agree; every 64-byte chunk looked
    at is charged whole"""
    n = len(t)
    slen = n - p
    common = max(0, min(slen, len(pat)))
    c = c0
    while c < common:
        k = min(WAVE, common - c)
        cnt[0] += k
        a, b = t[p + c:p + c + k], pat[c:c + k]
        if a != b:
            f = next(i for i in range(k) if a[i] != b[i])
            return (-1 if a[f] < b[f] else 1), c + f
        c += WAVE
    return (-1 if slen < len(pat) else (1 if slen > len(pat) else 0)), common


def descent(t, arr, pair, lp, pat, upper, cnt):
    N = len(t) + 1
    L, R, l, r = 0, 1 << lp, 0, 0
    for _ in range(lp):
        x = (L + R) >> 1
        c0 = -1
        if x > N:
            right, r = False, 0
        else:
            ll, rl = int(pair[x - 1, 0]), int(pair[x - 1, 1])
            if l >= r:
                if ll > l:
                    right = True
                elif ll < l:
                    right, r = False, ll
                else:
                    c0 = l
            else:
                if rl > r:
                    right = False
                elif rl < r:
                    right, l = True, rl
                else:
                    c0 = r
            if c0 >= 0:
                o, h = compare_from(t, int(arr[x - 1]), pat, c0, cnt)
                right = o < 0 or (upper and h == len(pat))
                if right:
                    l = h
                else:
                    r = h
        if right:
            L = x
        else:
            R = x
    return L, l, r


def esa_search(t, arr, pair, pat, bkt=None):
    """k_esa_search for one pattern -> ((contains, lo, hi, lcp_start, lcp_len), compared bytes)"""
    n = len(t)
    length = n + 1
    lp = log_p(n)
    cnt = [0]
    i, l, r = descent(t, arr, pair, lp, pat, False, cnt)
    j, _, _ = descent(t, arr, pair, lp, pat, True, cnt)
    plen = len(pat)
    empty = False
    if bkt is not None and plen > 1:
        idx = pat[0] * 257 + pat[1] + 2
        empty = bkt[idx - 1] == bkt[idx]
    elif bkt is not None and plen == 1:
        empty = bkt[pat[0] * 257] == bkt[pat[0] * 257 + 257]
    ls, ll = n, 0
    if empty:
        tlo, thi = int(bkt[pat[0] * 257]), int(bkt[pat[0] * 257 + 257])
        if thi > tlo:
            ls, ll = int(arr[tlo]), 1
    elif i < length and r == plen and n - int(arr[i]) == plen:
        ls, ll = int(arr[i]), plen
    elif 0 < i < length:
        ls, ll = (int(arr[i - 1]), l) if l > r else (int(arr[i]), r)
    elif i == 0:
        ls, ll = int(arr[0]), r
    else:
        ls, ll = int(arr[i - 1]), l
    return (j > i, i, j, ls, ll), cnt[0]


def plain_bytes(t, arr, pat):
    """text bytes k_search_batch's two binary searches (no bucket table) compare for pat, 64-byte chunks charged whole"""
    cnt = [0]
    lo, hi = 0, len(t) + 1
    while lo < hi:
        m = (lo + hi) // 2
        if compare_from(t, int(arr[m]), pat, 0, cnt)[0] < 0:
            lo = m + 1
        else:
            hi = m
    lo2, hi2 = lo, len(t) + 1
    while lo2 < hi2:
        m = (lo2 + hi2) // 2
        if compare_from(t, int(arr[m]), pat, 0, cnt)[1] == len(pat):
            lo2 = m + 1
        else:
            hi2 = m
    return cnt[0]


def bound(plen, n):
    return 2 * plen + 128 * log_p(n)


def patterns(t, rng, count=50):
    n = len(t)
    out = [b"", t, t + b"\x00", t + b"\xff", b"\x00" * (n + 3), bytes([t[0]]) if n else b"a"]
    while len(out) < count:
        kind = int(rng.integers(0, 4))
        if n == 0 or kind == 0:
            out.append(rng.integers(0, 256, int(rng.integers(1, 6))).astype(np.uint8).tobytes())
            continue
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(1, 300)))
        p = bytearray(t[a:b])
        if kind == 2:
            k = int(rng.integers(0, len(p)))
            p[k] = (p[k] + int(rng.integers(1, 256))) & 0xFF
        elif kind == 3:
            p += bytes([int(rng.integers(0, 256))])
        out.append(bytes(p))
    return out


def check_text(oracle, t, rng, count=50):
    t = bytes(t)
    arr = oracle.sais(t)
    pair = pair_table(kasai(t, arr))
    bkt = search_model.bucket_table(t)
    worst = 0.0
    for pat in patterns(t, rng, count):
        for bk in (None, bkt):
            got, used = esa_search(t, arr, pair, pat, bk)
            exp = search_model.search(t, arr, pat, bk)
            assert got == tuple(exp), (pat[:40], bk is None, got, exp)
            assert used <= bound(len(pat), len(t)), (pat[:40], used)
            worst = max(worst, used / bound(len(pat), len(t)))
    return worst


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_model_equals_the_reference_on_adversarial_cases(oracle, name):
    check_text(oracle, adversarial_cases()[name], np.random.default_rng(zlib.crc32(name.encode())), 40)


def test_model_equals_the_reference_on_random_texts(oracle):
    rng = np.random.default_rng(61)
    for _ in range(30):
        n = int(rng.integers(0, 3000))
        sigma = int(rng.choice([1, 2, 3, 4, 26, 256]))
        t = rng.integers(0, sigma, n).astype(np.uint8).tobytes()
        check_text(oracle, t, rng, 40)


def test_pair_table_at_the_virtual_ends():
    """Llcp of every node whose interval starts at the virtual -inf and Rlcp of every node whose interval reaches past N are 0"""
    for n in (0, 1, 2, 5, 6, 7, 1000, 4094, 4095, 4096):
        lcp = np.full(n + 1, 7, dtype=np.int64)
        lcp[0] = 0
        pair = pair_table(lcp)
        N = n + 1
        for x in range(1, N + 1):
            h = x & -x
            assert (pair[x - 1, 0] == 0) == (x - h == 0)
            assert (pair[x - 1, 1] == 0) == (x + h > N)


def test_model_work_bound_on_long_patterns(oracle):
    """one-byte text and a Fibonacci word: the descents compare close to plen bytes, where the plain binary search compares
    about plen per step"""
    for t in (b"a" * 20000, fibonacci_word(20)[:20000]):
        arr = oracle.sais(t)
        pair = pair_table(kasai(t, arr))
        for plen in (4096, 12000):
            pat = t[:plen]
            got, used = esa_search(t, arr, pair, pat)
            assert got == tuple(search_model.search(t, arr, pat))
            assert used <= bound(plen, len(t))
            if t[:1] * len(t) == t:
                assert plain_bytes(t, arr, pat) > 10 * bound(plen, len(t))
