"""Python restatement of the reference's search (test infrastructure only), and closed forms of periodic texts.

reference src/sa.rs:123-253: get_bucket, get_top_bucket, contains, search_all, search_lcp, with and without the bucket
table of enable_buckets.  `search(s, sa, pat, bkt)` answers one pattern the way sa_amd_index_search reports it:
(contains, lo, hi, lcp_start, lcp_len) with search_all(pat) == sa[lo:hi] (lo, hi are slots of the WHOLE array, also when
the search ran inside a bucket) and search_lcp(pat) == lcp_start..lcp_start + lcp_len.

Rust orders byte slices as Python orders `bytes`.  Every comparison of the pattern with a suffix s[p:] reads
s[p:p + len(pat) + 1] and no more, so the text may be a numpy array of any size: nothing is copied but those bytes.

`periodic_sa` is the suffix array of a prefix of w w w ... for a word w of distinct bytes (a one-byte text is |w| = 1):
a shorter suffix of the same phase is a prefix of a longer one, so the array is [n], then the phases by their first byte,
each phase's positions in descending order.  `periodic_mismatch` checks an array against it phase by phase in slices,
without building the expected array.
"""
import numpy as np


def _piece(s, p, k):
    """s[p:p + k] as bytes (p <= len(s))"""
    if isinstance(s, np.ndarray):
        return s[p:p + k].tobytes()
    return bytes(s[p:p + k])


def _ord(x, y):
    return (x > y) - (x < y)


def cmp_suffix(s, p, pat):
    """Ord of s[p..] against pat: -1, 0, +1 (reference: `s[i as usize..].cmp(pat)`)"""
    return _ord(_piece(s, p, len(pat) + 1), pat)


def lcp(pat, s, p):
    """lcp(pat, &s[p..]) of reference src/utils.rs"""
    x = _piece(s, p, len(pat))
    k = 0
    while k < len(x) and x[k] == pat[k]:
        k += 1
    return k


def get_bucket(s, sa, pat, bkt):                  # src/sa.rs:123-144
    if bkt is None:
        return 0, len(sa)
    if len(pat) > 1:
        idx = pat[0] * 257 + (pat[1] + 1) + 1
        return int(bkt[idx - 1]), int(bkt[idx])
    if len(pat) == 1:
        start = pat[0] * 257
        return int(bkt[start]), int(bkt[start + 257])
    return 0, 1


def get_top_bucket(s, sa, pat, bkt):              # src/sa.rs:146-160
    if bkt is None:
        return 0, len(sa)
    if len(pat) > 0:
        start = pat[0] * 257
        return int(bkt[start]), int(bkt[start + 257])
    return 0, 1


def _binary_search_by(lo, hi, order):
    """slice::binary_search_by over slots lo..hi: the first slot whose order is not Less (a slot of the whole array); the
    caller tells Ok from Err by looking at it.  Rust returns any match when there are several; the callers below either need
    only is_ok (contains) or compare whole suffixes, of which at most one equals the pattern (search_lcp), so the first
    match is as good as Rust's."""
    while lo < hi:
        m = lo + (hi - lo) // 2
        if order(m) < 0:
            lo = m + 1
        else:
            hi = m
    return lo


def contains(s, sa, pat, bkt=None):               # src/sa.rs:164-170
    lo, hi = get_bucket(s, sa, pat, bkt)
    m = len(pat)
    i = _binary_search_by(lo, hi, lambda k: _ord(_piece(s, int(sa[k]), m), pat))     # key: trunc(&s[i..], pat.len())
    return i < hi and _piece(s, int(sa[i]), m) == pat


def search_all(s, sa, pat, bkt=None):             # src/sa.rs:173-204 -> (lo, hi): the slots sa[lo:hi]
    lo, hi = get_bucket(s, sa, pat, bkt) if len(pat) > 0 else (0, len(sa))
    i, k = lo, hi
    while i < k:
        m = i + (k - i) // 2
        if cmp_suffix(s, int(sa[m]), pat) < 0:        # pat > &s[sa[m]..]
            i = m + 1
        else:
            k = m
    j, k = i, hi
    while j < k:
        m = j + (k - j) // 2
        if _piece(s, int(sa[m]), len(pat)) == pat:   # s[sa[m]..].starts_with(pat)
            j = m + 1
        else:
            k = m
    return i, j


def search_lcp(s, sa, pat, bkt=None):             # src/sa.rs:207-253 -> (start, len)
    n = len(s)
    lo, hi = get_bucket(s, sa, pat, bkt)
    if hi == lo:
        tlo, thi = get_top_bucket(s, sa, pat, bkt)
        if thi > tlo:
            return int(sa[tlo]), 1
        return n, 0
    i = _binary_search_by(lo, hi, lambda k: cmp_suffix(s, int(sa[k]), pat))
    if i < hi and cmp_suffix(s, int(sa[i]), pat) == 0:                    # Ok(i)
        return int(sa[i]), n - int(sa[i])
    if lo < i < hi:                                                        # Err(i), both neighbours inside the slice
        a, b = int(sa[i - 1]), int(sa[i])
        la, lb = lcp(pat, s, a), lcp(pat, s, b)
        return (a, la) if la > lb else (b, lb)
    p = int(sa[i]) if i == lo else int(sa[i - 1])
    return p, lcp(pat, s, p)


def search(s, sa, pat, bkt=None):
    """(contains, lo, hi, lcp_start, lcp_len) of one pattern, as sa_amd_index_search reports them"""
    pat = bytes(pat)
    lo, hi = search_all(s, sa, pat, bkt)
    st, ln = search_lcp(s, sa, pat, bkt)
    return contains(s, sa, pat, bkt), lo, hi, st, ln


def search_many(s, sa, pats, bkt=None):
    """search() over a list of patterns, as a dict of arrays in the layout of DeviceIndex.search"""
    rows = [search(s, sa, p, bkt) for p in pats]
    cols = list(zip(*rows)) if rows else [()] * 5
    return {"contains": np.array(cols[0], dtype=bool), "lo": np.array(cols[1], dtype=np.uint32),
            "hi": np.array(cols[2], dtype=np.uint32), "lcp_start": np.array(cols[3], dtype=np.uint32),
            "lcp_len": np.array(cols[4], dtype=np.uint32)}


def bucket_table(s):
    """enable_buckets (src/sa.rs:89-119) for small texts: bigram counts + inclusive prefix sum"""
    b = np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s
    cnt = np.zeros(256 * 257 + 1, dtype=np.int64)
    cnt[0] = 1
    if b.size:
        np.add.at(cnt, b[:-1].astype(np.int64) * 257 + b[1:].astype(np.int64) + 2, 1)
        cnt[int(b[-1]) * 257 + 1] += 1
    return np.cumsum(cnt).astype(np.uint32)


# ---- naive checkers restated from the reference's own tests (src/tests.rs:104-132) ----

def naive_lcp(a, b):
    k = 0
    while k < len(a) and k < len(b) and a[k] == b[k]:
        k += 1
    return k


def naive_contains(s, pat):
    return any(pat == s[i:min(len(s), i + len(pat))] for i in range(0, max(len(s) - len(pat), 0) + 1))


def naive_search_all(s, pat):
    return [i for i in range(0, max(len(s) - len(pat), 0) + 1) if pat == s[i:min(len(s), i + len(pat))]]


def naive_search_lcp(s, pat):
    best = 0
    for i in range(len(s) + 1):
        best = max(best, naive_lcp(pat, s[i:]))
    return pat[:best]


# ---- periodic texts ----

def periodic_text(w, n):
    """the first n bytes of w w w ..."""
    return np.resize(np.frombuffer(bytes(w), dtype=np.uint8), n) if n else np.zeros(0, dtype=np.uint8)


def _phases(w, n):
    """(phase r, its last position < n, its count) in suffix-array order: by the phase's byte"""
    w = bytes(w)
    k = len(w)
    assert k >= 1 and len(set(w)) == k, "the closed form needs a word of distinct bytes"
    out = []
    for r in sorted(range(k), key=lambda r: w[r]):
        if r < n:
            last = r + ((n - 1 - r) // k) * k
            out.append((r, last, (last - r) // k + 1))
    return out


def periodic_sa(w, n):
    """suffix array (n + 1 entries) of periodic_text(w, n)"""
    parts = [np.array([n], dtype=np.uint32)]
    for r, last, cnt in _phases(w, n):
        parts.append(np.arange(last, r - 1, -len(w), dtype=np.int64).astype(np.uint32))
    return np.concatenate(parts)


def periodic_mismatch(arr, w, n, chunk=1 << 24):
    """first slot where arr differs from periodic_sa(w, n), or None; compares slices of at most `chunk` entries"""
    k = len(w)
    if arr.size != n + 1:
        return min(arr.size, n + 1)
    if int(arr[0]) != n:
        return 0
    slot = 1
    for r, last, cnt in _phases(w, n):
        for c0 in range(0, cnt, chunk):
            c1 = min(cnt, c0 + chunk)
            exp = np.arange(last - c0 * k, last - c1 * k, -k, dtype=np.int64)
            got = arr[slot + c0:slot + c1]
            bad = np.flatnonzero(got.astype(np.int64) != exp)
            if bad.size:
                return slot + c0 + int(bad[0])
        slot += cnt
    return None
