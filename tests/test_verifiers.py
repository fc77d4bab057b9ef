"""Every suffix-array verifier against near-miss arrays (reference src/sa.rs:72-84, `check_integrity`).

Above a few tens of MiB the suite trusts verifiers instead of comparing with the oracle's SA-IS, so each verifier here is
fed the arrays a subtly broken builder would produce.  No verifier is trusted for the expected answer: the suffix array of
a text is unique, so an array whose entries are all <= n is right exactly when it equals oracle.sais(text), and an array
holding an entry > n is refused as out of range (SA_AMD_ERANGE / IndexError: the reference panics on the slice index).

Families, one defect per array:
  (a) h-order: sorted by the first h bytes only, ties by ascending / descending position
  (b) the end of the text sorted as +inf (a proper prefix after the longer suffix); cyclic rotation order
  (c) one tie group at depth h reversed or rotated (the largest one, and one of two members)
  (d) the right array for the wrong text: the array of a text that differs in one byte
  (e) adjacent swaps at the slots where the verifiers take separate paths: slots 1/2 and n-1/n, first-byte boundaries,
      the first lane of a wave (i = 1 mod 64), the workgroup edges of k_ci_check_shared (i = 1 mod 2048), the grid-stride
      wrap of the small form (16 384 x 256 slots), the chunk edges of oracle_verify_sa_mt, the slot of suffix n - 1
  (f) duplicates: 0 or n - 1 missing, a neighbour's value twice, the empty suffix twice, slot 0 without it
  (g) entries out of range: n + 1, 2^31, 0xffffffff at slots 0, 1, n and a first-lane slot

CPU part (no marker): oracle_verify_sa, oracle_verify_sa_mt at 1, 3 and 16 threads, the numpy fallback of from_parts in its
literal and its vectorised form and, where the cost allows, oracle_check_integrity (the literal restatement).
GPU part: sa_amd_check_integrity_device with the streaming work block, with the small one, and with a dSA that is not
16-byte aligned (the small form, taken silently), each after the work block was filled with 0xff and with random bytes;
sa_amd_check_integrity; sa_amd_index_check_integrity on an index made from the parts; SuffixArray.from_parts.
"""
import ctypes

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus

WAVE = 64
CI_BLOCK = 2048                      # slots per workgroup of k_ci_check_shared (CI_THREADS * CI_ITEMS)
GRID_WRAP = 16384 * 256              # first slot the small form reaches on its second grid-stride lap
MT_THREADS = (1, 3, 16)
ERANGE = -6

SMALL_N = (0, 1, 2, 3, 63, 64, 65, 66, 2047, 2048, 2049, 2050)
MID_N = (1 << 20) + 3
WRAP_N = GRID_WRAP + 5
BIG_N = (64 << 20) + 3

PERIOD_5 = b"\x80\x00\xff\x01\x7f"
KINDS = ("one_byte", "two_symbols", "dna", "all_256", "english", "period_5", "gappy_256", "extremes")
LOW_LCP = ("two_symbols", "dna", "all_256", "gappy_256", "extremes")     # oracle_check_integrity affordable at ~1 MiB


def make_text(kind, n, seed=11):
    rng = np.random.default_rng(seed * 100_003 + n)
    if kind == "one_byte":
        return np.full(n, 0x61, dtype=np.uint8)
    if kind == "two_symbols":
        return rng.choice(np.array([0x61, 0x62], dtype=np.uint8), n)
    if kind == "dna":
        return corpus.dna(n, seed)
    if kind == "all_256":                       # every byte value, 0x00 and 0xff planted for short texts
        t = corpus.uniform(n, seed)
        if n >= 3:
            t[n // 3], t[2 * n // 3] = 0x00, 0xff
        return t
    if kind == "english":
        return corpus.english_corpus(n, seed)
    if kind == "period_5":
        return np.resize(np.frombuffer(PERIOD_5, dtype=np.uint8), n)
    if kind == "gappy_256":                     # 0x00 and most values absent, 0xff present: many of the 257 starts coincide
        vals = np.r_[np.arange(0x10, 0x40), np.arange(0x90, 0xa0), 0xff].astype(np.uint8)
        return rng.choice(vals, n)
    if kind == "extremes":                      # only 0x00 and 0xff
        return rng.choice(np.array([0x00, 0xff], dtype=np.uint8), n)
    raise ValueError(kind)


def expected(arr, good):
    """1 / 0 / ERANGE: the answer every product form must give"""
    n = good.size - 1
    if int(arr.max()) > n:
        return ERANGE
    return int(np.array_equal(arr, good))


# ---- near-miss families ----------------------------------------------------------------------------------------------

def _padded(t, h):
    """symbols + 1, then h + 1 zeros: the end of the text sorts first"""
    p = np.zeros(t.size + h + 1, dtype=np.uint16)
    p[:t.size] = t.astype(np.uint16) + 1
    return p


def h_order(t, h, descending):
    """(a) order by the first h bytes, ties broken by ascending (or descending) position: LSD passes of a stable sort"""
    n = t.size
    order = np.arange(n, -1, -1, dtype=np.int64) if descending else np.arange(n + 1, dtype=np.int64)
    p = _padded(t, h)
    for k in range(h - 1, -1, -1):
        order = order[np.argsort(p[order + k], kind="stable")]
    return order.astype(np.uint32)


def end_last_order(t):
    """(b) the end of the text as +inf: a suffix that is a proper prefix of another sorts after it (two bytes per symbol,
    the terminator 0x0100 above every symbol 0x00XX)"""
    n = t.size
    b = t.astype(">u2").tobytes()
    keys = [b[2 * i:] + b"\x01\x00" for i in range(n + 1)]
    return np.array(sorted(range(n + 1), key=keys.__getitem__), dtype=np.uint32)


def cyclic_order(oracle, t):
    """(b) the order of the rotations: the suffix array of t + t restricted to positions < n, the empty suffix first"""
    n = t.size
    c = oracle.sais(np.concatenate([t, t]))[1:]
    return np.r_[np.uint32(n), c[c < n]].astype(np.uint32)


def tie_groups(t, good, h):
    """(start slot, size) of the runs of slots 1..n whose suffixes share their first h bytes"""
    n = t.size
    p = _padded(t, h)
    pos = good[1:].astype(np.int64)
    key = p[pos].astype(np.int64)
    for k in range(1, h):
        key = key * 257 + p[pos + k]
    cut = np.flatnonzero(np.diff(key)) + 1
    starts = np.r_[0, cut]
    sizes = np.diff(np.r_[starts, n])
    return starts + 1, sizes


def structural_slots(t, good, rng=None, per_kind=None):
    """(e) slots p for a swap of p and p + 1.  per_kind: how many first-lane / workgroup-edge slots to sample (None: all)"""
    n = t.size
    if n == 0:
        return []
    ps = {0, 1, n - 1}
    fb = t[good[1:].astype(np.int64)]
    bounds = np.flatnonzero(np.diff(fb)) + 2                       # slot i: the first byte changes between i - 1 and i
    lane0 = np.arange(1, n + 1, WAVE)
    edges = np.arange(1, n + 1, CI_BLOCK)
    if per_kind is not None:
        if bounds.size:
            bounds = np.unique(np.r_[bounds[:3], bounds[-3:], rng.choice(bounds, min(per_kind, bounds.size), replace=False)])
        lane0 = np.unique(np.r_[lane0[:3], lane0[-3:], rng.choice(lane0, min(per_kind, lane0.size), replace=False)])
        edges = np.unique(np.r_[edges[:2], edges[-2:], rng.choice(edges, min(per_kind, edges.size), replace=False)])
    ps.update(int(i) - 1 for i in bounds)
    for i in lane0.tolist():
        ps.update((i - 1, i))
    for i in edges.tolist():
        ps.update((i - 2, i - 1, i))
    ps.update((GRID_WRAP - 1, GRID_WRAP))
    for threads in MT_THREADS + (7,):
        per = -(-(n + 1) // threads)
        ps.update(k * per - 1 for k in range(1, threads))
    r = int(np.flatnonzero(good == n - 1)[0])                       # suffix n - 1: its next suffix is the empty one
    ps.update((r - 1, r))
    return sorted(p for p in ps if 0 <= p <= n - 1)


def near_misses(oracle, t, good, full=True, rng=None):
    """(label, array) pairs; `full=False` for texts of MiBs: fewer depths, sampled slots, no quadratic families"""
    n = t.size
    yield "good", good
    for h in (1, 2, 4, 8, 16, 32) if full else (1, 2):
        if h <= max(n, 1):
            yield f"a:h{h}:asc", h_order(t, h, False)
            yield f"a:h{h}:desc", h_order(t, h, True)
    if full:
        e = end_last_order(t)
        yield "b:end_last", e
        yield "b:end_last_empty_first", np.r_[np.uint32(n), e[e != n]].astype(np.uint32)
        yield "b:cyclic", cyclic_order(oracle, t)
    for h in (1, 2):
        if n < 2:
            break
        starts, sizes = tie_groups(t, good, h)
        g = int(np.argmax(sizes))
        s0, sz = int(starts[g]), int(sizes[g])
        if sz >= 2:
            a = good.copy(); a[s0:s0 + sz] = good[s0:s0 + sz][::-1]
            yield f"c:h{h}:largest_reversed", a
            a = good.copy(); a[s0:s0 + sz] = np.roll(good[s0:s0 + sz], 1)
            yield f"c:h{h}:largest_rotated", a
        two = np.flatnonzero(sizes == 2)
        if two.size:
            s2 = int(starts[two[two.size // 2]])
            a = good.copy(); a[s2], a[s2 + 1] = good[s2 + 1], good[s2]
            yield f"c:h{h}:pair_reversed", a
    if n >= 1:
        a = good.copy(); a[1:] = np.roll(good[1:], 1)
        yield "c:all_rotated", a
    if full:
        where = sorted({0, 1, 2, 3, n // 2, 4 * (n // 8) + 1, n - 1})
        flips = (lambda b: (b + 1) & 0xff, lambda b: b ^ 0x80)
    else:
        where, flips = sorted({0, n // 2, n - 1}), ((lambda b: (b + 1) & 0xff),)
    for j in where:
        if 0 <= j < n:
            for k, f in enumerate(flips):
                t2 = t.copy(); t2[j] = f(int(t[j]))
                yield f"d:byte{j}:{k}", oracle.sais(t2)
    for p in structural_slots(t, good, rng, None if full else 8):
        a = good.copy(); a[p], a[p + 1] = good[p + 1], good[p]
        yield f"e:swap{p}", a
    if n >= 1:
        rank = np.empty(n + 1, dtype=np.int64); rank[good] = np.arange(n + 1)
        for v in sorted({0, n - 1}):                                # v missing: its slot holds a neighbour's value
            r = int(rank[v])
            a = good.copy(); a[r] = good[r + 1] if r < n else good[r - 1]
            yield f"f:missing{v}", a
        for p in sorted({1, n // 2, WAVE + 1, n - 1}):
            if 1 <= p < n:
                a = good.copy(); a[p] = good[p + 1]
                yield f"f:dup_right{p}", a
                a = good.copy(); a[p + 1] = good[p]
                yield f"f:dup_left{p}", a
        for p in sorted({1, n}):
            a = good.copy(); a[p] = n
            yield f"f:empty_twice{p}", a
        a = good.copy(); a[0] = good[1]
        yield "f:empty_missing", a
    for v in (n + 1, 1 << 31, 0xffffffff):
        for p in sorted({0, 1, n, WAVE + 1}):
            if p <= n:
                a = good.copy(); a[p] = v
                yield f"g:{v:#x}@{p}", a


# ---- the CPU verifiers -----------------------------------------------------------------------------------------------

def fallback(fn, t, arr):
    try:
        return int(fn(t, arr))
    except IndexError:
        return ERANGE


def check_cpu(oracle, t, arr, exp, label, literal_ref):
    n = t.size
    want = int(exp == 1)
    assert oracle.verify(t, arr) == want, ("verify", label)
    for threads in MT_THREADS:
        assert oracle.verify_mt(t, arr, threads) == want, ("verify_mt", threads, label)
    assert fallback(sa._check_integrity, t, arr) == exp, ("fallback", label)
    if exp != ERANGE:
        assert int(sa._check_integrity_linear(t, arr)) == exp, ("fallback linear", label)
        if n <= 66:
            assert int(sa._check_integrity_literal(t, arr)) == exp, ("fallback literal", label)
    if literal_ref:                                                 # (n = 0: the reference never reads the entry)
        ref = 1 if n == 0 else {1: 1, 0: 0, ERANGE: -1}[exp]
        assert oracle.check_integrity(t, arr) == ref, ("oracle_check_integrity", label)


def run_cpu(oracle, t, full, literal_ref, seed=0):
    good = oracle.sais(t)
    seen = 0
    for label, arr in near_misses(oracle, t, good, full, np.random.default_rng(seed)):
        check_cpu(oracle, t, arr, expected(arr, good), label, literal_ref)
        seen += 1
    return seen


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_verifiers_small(oracle, kind, n):
    t = make_text(kind, n)
    assert run_cpu(oracle, t, True, True) >= 1


@pytest.mark.parametrize("kind", ("one_byte", "dna", "all_256", "english", "gappy_256"))
def test_cpu_verifiers_large(oracle, kind):
    t = make_text(kind, MID_N)
    assert run_cpu(oracle, t, False, kind in LOW_LCP, seed=MID_N) > 20


def test_verify_mt_chunk_edges(oracle):
    """a swap across the boundary of every thread's chunk (slots t * per - 1 and t * per), one at a time, at thread counts
    that do and do not divide n + 1"""
    for n in (2047, 2048, 4999):
        t = make_text("all_256", n)
        good = oracle.sais(t)
        for threads in (2, 3, 7, 16, 64):
            per = -(-(n + 1) // threads)
            for k in range(1, threads):
                p = k * per - 1
                if p + 1 > n:
                    break
                a = good.copy(); a[p], a[p + 1] = good[p + 1], good[p]
                assert oracle.verify_mt(t, a, threads) == 0, (n, threads, p)
            assert oracle.verify_mt(t, good, threads) == 1


def test_empty_text(oracle):
    """n = 0: [0] is the only suffix array; any other single entry is out of range for every product form (the
    reference's loop never reads it and says true: the product diverges on purpose, include/suffix_array_amd.h)"""
    t = np.zeros(0, dtype=np.uint8)
    assert sa._check_integrity(t, np.array([0], dtype=np.uint32)) is True
    assert sa.SuffixArray.from_parts(b"", [0]) is not None
    assert oracle.check_integrity(t, [0]) == 1 and oracle.verify(t, [0]) == 1
    for v in (1, 5, 1 << 31, 0xffffffff):
        a = np.array([v], dtype=np.uint32)
        assert oracle.check_integrity(t, a) == 1                    # the literal reference: true
        assert oracle.verify(t, a) == 0 and oracle.verify_mt(t, a, 3) == 0
        with pytest.raises(IndexError):
            sa._check_integrity(t, a)
        with pytest.raises(IndexError):
            sa.SuffixArray.from_parts(b"", a)                       # the GPU check or the fallback: the same answer


# ---- the GPU forms ---------------------------------------------------------------------------------------------------

class _Hip:
    def __init__(self):
        h = ctypes.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        h.hipFree.argtypes = [ctypes.c_void_p]
        h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        self.h = h

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.h.hipMalloc(ctypes.byref(p), nbytes) == 0
        return p.value


class DeviceForms:
    """device buffers for one text: the text, the array at a 256-byte aligned address and at +4 bytes, the work block of
    the streaming form, and random bytes to fill it with"""

    def __init__(self, t, seed):
        self.hip = _Hip()
        self.L = sa.lib()
        self.t = t
        self.n = n = int(t.size)
        self.big = int(self.L.sa_amd_check_integrity_work_bytes(n))
        self.small = 4 * (n + 1) + 256
        assert self.big >= self.small
        self.ptrs = []
        alloc = lambda b: self.ptrs.append(self.hip.malloc(b)) or self.ptrs[-1]     # noqa: E731
        self.dt = alloc(n + 64)
        self.ds = alloc(4 * (n + 1) + 64)
        self.ds4 = alloc(4 * (n + 1) + 64) + 4
        self.work = (alloc(self.big + 512) + 255) & ~255
        self.chunk = min(self.big, 16 << 20)
        self.rnd = alloc(2 * self.chunk)
        rng = np.random.default_rng(seed)
        r = rng.integers(0, 256, 2 * self.chunk, dtype=np.uint8)
        assert self.hip.h.hipMemcpy(self.rnd, r.ctypes.data, r.size, 1) == 0
        if n:
            assert self.hip.h.hipMemcpy(self.dt, t.ctypes.data, n, 1) == 0
        self.rng = rng

    def close(self):
        for p in self.ptrs:
            self.hip.h.hipFree(p)
        self.ptrs = []

    def _fill(self, how):
        if how == "ff":
            assert self.hip.h.hipMemset(self.work, 0xff, self.big) == 0
            return
        o = int(self.rng.integers(0, self.chunk))
        for off in range(0, self.big, self.chunk):
            ln = min(self.chunk, self.big - off)
            assert self.hip.h.hipMemcpy(self.work + off, self.rnd + o, ln, 3) == 0

    def answers(self, arr):
        n, L = self.n, self.L
        out = {}
        assert self.hip.h.hipMemcpy(self.ds, arr.ctypes.data, 4 * (n + 1), 1) == 0
        assert self.hip.h.hipMemcpy(self.ds4, arr.ctypes.data, 4 * (n + 1), 1) == 0
        for how in ("ff", "random"):
            for name, ds, wb in (("streaming", self.ds, self.big), ("small", self.ds, self.small),
                                 ("unaligned", self.ds4, self.big)):
                self._fill(how)
                out[f"{name}/{how}"] = L.sa_amd_check_integrity_device(self.dt, n, ds, self.work, wb, None)
        out["host"] = L.sa_amd_check_integrity(self.t.ctypes.data, n, arr.ctypes.data, arr.size)
        ix = sa.DeviceIndex(self.t, arr)                            # (no search on an index made from a wrong array)
        try:
            out["index"] = L.sa_amd_index_check_integrity(ix._h)
        finally:
            ix.close()
        try:
            out["from_parts"] = int(sa.SuffixArray.from_parts(self.t, arr) is not None)
        except IndexError:
            out["from_parts"] = ERANGE
        return out


def run_gpu(oracle, t, full, seed=0, cpu_too=False):
    good = oracle.sais(t)
    dev = DeviceForms(t, seed)
    seen = 0
    try:
        for label, arr in near_misses(oracle, t, good, full, np.random.default_rng(seed)):
            exp = expected(arr, good)
            got = dev.answers(arr)
            bad = {k: v for k, v in got.items() if v != exp}
            assert not bad, (label, exp, bad)
            if cpu_too:
                assert oracle.verify_mt(t, arr, 16) == int(exp == 1), label
            seen += 1
    finally:
        dev.close()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_verifiers_small(oracle, kind, n):
    t = make_text(kind, n)
    assert run_gpu(oracle, t, True, seed=n) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(k, MID_N) for k in ("one_byte", "dna", "all_256", "english", "gappy_256", "period_5")]
                         + [(k, WRAP_N) for k in ("all_256", "one_byte", "english")])
def test_gpu_verifiers_large(oracle, kind, n):
    t = make_text(kind, n)
    assert run_gpu(oracle, t, False, seed=n) > 20


@pytest.mark.gpu
def test_gpu_verifiers_64_mib(oracle):
    """the stride loops of the streaming form (k_ci_range, k_ci_first_bytes grids capped at 16 384 workgroups), with
    oracle_verify_sa_mt beside it on every array"""
    t = make_text("english", BIG_N)
    assert run_gpu(oracle, t, False, seed=64, cpu_too=True) > 20


# sizes at which the window arithmetic of the streaming form's binned inverse permutation changes (scatter_binned,
# host/pipeline.hpp: window 2^10 entries for these sizes, 8 bits per pass above it): 1023 has no bit above the window, so a
# two-pass request is answered by the one-pass form; 1024 is the first size with one; 65 537 has 17 bits, the first pass
# covers them all and the second is skipped; 300 000 has 19, both passes run
LEVEL_N = (1023, 1024, 65537, 300000)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", (1, 2))
@pytest.mark.parametrize("n", LEVEL_N)
@pytest.mark.parametrize("kind", ("dna", "english"))
def test_gpu_verifiers_scatter_levels(oracle, monkeypatch, kind, n, levels):
    """the streaming form with its inverse permutation binned by one radix pass and by two (SA_AMD_SCATTER_LEVELS): by size it
    takes one below 2^25 entries, so only test_gpu_verifiers_64_mib reaches the two-pass form with this form's own buffers.
    run_gpu drives sa_amd_check_integrity_device itself with a 256-byte aligned block of sa_amd_check_integrity_work_bytes(n)
    bytes ("streaming/*"); that this is the streaming form is checked first: the call writes behind the 4 (n + 1) + 256 bytes
    that are all the small form touches."""
    monkeypatch.setenv("SA_AMD_SCATTER_LEVELS", str(levels))
    t = make_text(kind, n)
    good = oracle.sais(t)
    dev = DeviceForms(t, n)
    try:
        dev._fill("ff")
        assert dev.hip.h.hipMemcpy(dev.ds, good.ctypes.data, 4 * (n + 1), 1) == 0
        assert dev.L.sa_amd_check_integrity_device(dev.dt, n, dev.ds, dev.work, dev.big, None) == 1
        tail = np.empty(dev.big - dev.small, dtype=np.uint8)
        assert dev.hip.h.hipMemcpy(tail.ctypes.data, dev.work + dev.small, tail.size, 2) == 0
        assert (tail != 0xff).any()
    finally:
        dev.close()
    assert run_gpu(oracle, t, n <= 2050, seed=n) > 20


@pytest.mark.gpu
def test_gpu_empty_text():
    """n = 0 on every GPU form: [0] is right, any other single entry is out of range (see test_empty_text)"""
    t = np.zeros(0, dtype=np.uint8)
    dev = DeviceForms(t, 0)
    try:
        got = dev.answers(np.array([0], dtype=np.uint32))
        assert set(got.values()) == {1}, got
        for v in (1, 5, 1 << 31, 0xffffffff):
            got = dev.answers(np.array([v], dtype=np.uint32))
            assert set(got.values()) == {ERANGE}, (v, got)
    finally:
        dev.close()
