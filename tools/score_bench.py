"""DESIGN.md section 22, measured: infgram_score over the device index (kernels/score.hpp) beside the only route a caller had
before it -- sa_amd_index_infgram on one explicit prompt per position (up to max_len bytes each) and the look-up of the query's
byte in each listing -- on the same index, in the same process, with the answers compared in full.

python tools/score_bench.py [--index-mib 256] [--query-mib 1,16] [--max-lens 32,256,4096] [--min-counts 1,2] [--reps 5]
                            [--baseline-positions 65536] [--caps 0,16,64,256] [--out profiles/score_table.txt]

Texts: the English-like corpus of bench.py (corpus.english_corpus(n, 3)) and corpus.dna(n, 4).  Queries: held-out text (the same
generator, another seed) and a slice of the text with 1 % of its bytes substituted.  Times are the median of --reps calls after
a warm-up with min..max: host to host (query up, six arrays down into arrays allocated once), and device-resident (query and
outputs in device memory, the call blocks until done).  The explicit prompts of a whole query do not fit (m max_len bytes), so
the old route runs on the first --baseline-positions positions and both sides are reported per position."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import suffix_array_amd as sa
from suffix_array_amd import corpus

NAMES = ("s", "lo", "hi", "at_end", "nlo", "nhi")


def spread(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}..{max(xs):.3f})"


def timed(fn, reps):
    out = []
    for _ in range(reps + 1):                                         # (the first call is the warm-up; every call blocks until it is done)
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


class Hip:
    """device buffers by hipMalloc of the runtime the library itself uses"""

    def __init__(self):
        self.h = ctypes.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.h.hipFree.argtypes = [ctypes.c_void_p]
        self.h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.held = []

    def alloc(self, size):
        p = ctypes.c_void_p()
        assert self.h.hipMalloc(ctypes.byref(p), max(int(size), 256)) == 0
        self.held.append(p.value)
        return p.value

    def up(self, dst, arr):
        assert self.h.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, 1) == 0

    def down(self, arr, src):
        assert self.h.hipMemcpy(arr.ctypes.data, src, arr.nbytes, 2) == 0

    def free(self):
        for p in self.held:
            self.h.hipFree(p)
        self.held = []


class Caller:
    def __init__(self, ix):
        self.ix, self.L = ix, sa.lib()
        self.bufs = {}

    def out(self, m):
        """the six result arrays of a query length, allocated and touched once"""
        if m not in self.bufs:
            self.bufs.clear()
            self.bufs[m] = {k: np.zeros(m, dtype=np.uint8 if k == "at_end" else np.uint32) for k in NAMES}
        return self.bufs[m]

    def score(self, q, min_count, max_len):
        o = self.out(q.size)
        assert self.L.sa_amd_index_infgram_score(self.ix._h, q.ctypes.data, q.size, None, 0, min_count, max_len, *(o[k].ctypes.data for k in NAMES)) == 0
        return o

    def old_route(self, q, count, min_count, max_len):
        """what the parent commit offers: one prompt per position, then the query's byte looked up in each listing"""
        j = np.arange(count, dtype=np.int64)
        lens = np.minimum(j, max_len)
        off = np.zeros(count + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        head = min(count, max_len + 1)                                # prompts that start at 0: position j has j bytes
        parts = [q[np.repeat(-off[:head], lens[:head]) + np.arange(off[head])]]
        if count > head:                                              # the others are the windows q[j - max_len .. j)
            parts.append(np.lib.stride_tricks.sliding_window_view(q[1:count - 1], max_len).reshape(-1))
        data = np.ascontiguousarray(np.concatenate(parts)) if off[-1] else np.zeros(1, dtype=np.uint8)
        assert data.size == max(int(off[-1]), 1)
        s, lo, hi = (np.zeros(count, dtype=np.uint32) for _ in range(3))
        ae = np.zeros(count, dtype=np.uint8)
        loff = np.zeros(count + 1, dtype=np.int64)
        cap = 256 * count
        b, c = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint32)
        tot = ctypes.c_int64(0)
        assert self.L.sa_amd_index_infgram(self.ix._h, data.ctypes.data, off.ctypes.data, count, min_count, max_len, s.ctypes.data, lo.ctypes.data,
                                           hi.ctypes.data, ae.ctypes.data, loff.ctypes.data, b.ctypes.data, c.ctypes.data, cap, ctypes.byref(tot)) == 0
        k = int(tot.value)
        row = np.repeat(j, np.diff(loff))
        byte = q[:count][row]
        less = np.bincount(row, weights=np.where(b[:k] < byte, c[:k], 0), minlength=count).astype(np.int64)
        same = np.bincount(row, weights=np.where(b[:k] == byte, c[:k], 0), minlength=count).astype(np.int64)
        nlo = lo.astype(np.int64) + ae + less
        return {"s": s, "lo": lo, "hi": hi, "at_end": ae, "nlo": nlo, "nhi": nlo + same}, int(off[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mib", type=int, default=256)
    ap.add_argument("--query-mib", default="1,16")
    ap.add_argument("--max-lens", default="32,256,4096")
    ap.add_argument("--min-counts", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-positions", type=int, default=65536)
    ap.add_argument("--caps", default="0,16,64,256")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = args.index_mib << 20
    sizes = [int(x) << 20 for x in args.query_mib.split(",")]
    max_lens = [int(x) for x in args.max_lens.split(",")]
    min_counts = [int(x) for x in args.min_counts.split(",")]
    caps = [int(x) for x in args.caps.split(",")]
    say(f"tools/score_bench.py: library {os.path.basename(sa.library_path())}; indexes of {args.index_mib} MiB; ms, median of {args.reps} calls after a "
        f"warm-up (min..max); the old route (infgram on explicit prompts + look-up) runs on the first {args.baseline_positions} positions, both "
        f"sides per position in us; default group cap {sa.SCORE_GROUP_CAP_DEFAULT}, 8 lanes a position")
    beaten = True
    hip = Hip()
    for label, make in (("English-like", corpus.english_corpus), ("DNA", corpus.dna)):
        t = make(n, 3 if label != "DNA" else 4)
        held = make(max(sizes), 5 if label != "DNA" else 6)
        ix = sa.DeviceIndex(t)
        call = Caller(ix)
        rng = np.random.default_rng(7)
        say(f"\n== {label}, {n} bytes ==")
        for m in sizes:
            a = int(rng.integers(0, n - m))
            sl = t[a:a + m].copy()
            hit = rng.random(m) < 0.01
            sl[hit] = rng.integers(0, 256, int(hit.sum())).astype(np.uint8)
            for qname, q in ((f"held-out {m >> 20} MiB", np.ascontiguousarray(held[:m])), (f"slice {m >> 20} MiB, 1 % substituted", sl)):
                dQ, dW = hip.alloc(m + 16), hip.alloc(sa.score_work_bytes(m, 1))
                dO = [hip.alloc(m * (1 if k == "at_end" else 4)) for k in NAMES]
                hip.up(dQ, q)
                for max_len in max_lens:
                    for min_count in min_counts:
                        ours = timed(lambda: call.score(q, min_count, max_len), args.reps)
                        got = {k: v.copy() for k, v in call.score(q, min_count, max_len).items()}
                        st = sa.last_score_stats()
                        dev = timed(lambda: sa.infgram_score_device_ptr(ix, dQ, m, min_count, max_len, *dO, dW, sa.score_work_bytes(m, 1)), args.reps)
                        for k, p in zip(NAMES, dO):                    # the device form's answers are the host form's
                            back = np.zeros_like(got[k])
                            hip.down(back, p)
                            assert np.array_equal(back, got[k]), k
                        sub = min(m, args.baseline_positions)
                        base = timed(lambda: call.old_route(q, sub, min_count, max_len), max(1, args.reps // 2))
                        old, prompt_bytes = call.old_route(q, sub, min_count, max_len)
                        for k in NAMES:
                            assert np.array_equal(old[k].astype(np.int64), got[k][:sub].astype(np.int64)), f"the old route's {k} differs"
                        us_ours, us_dev, us_base = (statistics.median(x) * 1e3 for x in (ours, dev, base))
                        us_ours, us_dev, us_base = us_ours / m, us_dev / m, us_base / sub
                        beaten &= us_ours < us_base
                        say(f"{qname}, max_len {max_len}, min_count {min_count}: host {spread(ours)} ms = {us_ours:.4f} us/pos; device {spread(dev)} ms = "
                            f"{us_dev:.4f} us/pos; old route on {sub} positions ({prompt_bytes} prompt bytes) {spread(base)} ms = {us_base:.4f} us/pos; "
                            f"ratio {us_base / us_ours:.1f}x; mean S {got['s'].mean():.1f}, searches/pos {st['range_searches'] / m:.2f}, long "
                            f"{st['long_positions']}, p = 0 at {st['zero_positions']}, compared bytes/pos {st['compared_bytes'] / m:.0f}")
                if m == sizes[0]:
                    row = []
                    for cap in caps:                                  # the A/B of the group cap, device-resident, max_len 4096
                        prev = sa.score_set_group_cap(cap)
                        try:
                            row.append(f"{cap}: {spread(timed(lambda: sa.infgram_score_device_ptr(ix, dQ, m, 1, max_lens[-1], *dO, dW, sa.score_work_bytes(m, 1)), args.reps))}")
                        finally:
                            sa.score_set_group_cap(prev)
                    say(f"   {qname}, max_len {max_lens[-1]}, by group cap (device ms): " + "; ".join(row))
                hip.free()
        ix.close()
    say(f"\nevery row faster than the old route: {'yes' if beaten else 'NO'}")
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
