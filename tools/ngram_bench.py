"""DESIGN.md section 21, measured: next_bytes and infgram over the device index (kernels/ngram.hpp) beside the only routes a
caller had before them -- sa_amd_index_search over the 257-pattern expansion of every context (the context, and the context plus
each byte), and a host loop of bisection over sa_amd_index_search for the back-off -- on the same index, in the same process,
with the answers compared.

python tools/ngram_bench.py [--index-mib 256] [--contexts 65536,1048576] [--prompts 65536] [--baseline-contexts 4096] [--reps 5]
                            [--caps 256,1024,4096,16384] [--out profiles/ngram_table.txt]

Texts: the English-like corpus of bench.py (corpus.english_corpus(n, 3)) and corpus.dna(n, 4).  Contexts: 8 to 32 bytes sampled
from the text, and the 256 single-byte contexts.  Prompts: 256 bytes of held-out text (the same generator, another seed) and
slices of the text with 1 % of their bytes substituted.  Times are host to host (patterns up, answers down into result arrays
allocated once per batch shape), the median of --reps calls after a warm-up with min..max.  The expansion of C contexts is 257 C patterns; it is run on the first --baseline-contexts
contexts of a batch and both sides are reported per context, so the ratio compares like with like."""
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


def spread(xs):
    return f"{statistics.median(xs):10.3f} ({min(xs):.3f}..{max(xs):.3f})"


def timed(fn, reps):
    out = []
    for _ in range(reps + 1):                                         # (the first call is the warm-up; every call blocks until its answers are on the host)
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def gather(t, starts, lens):
    """the batch of t[starts[q] : starts[q] + lens[q]] -> (data, off)"""
    off = np.zeros(starts.size + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    idx = np.repeat(starts - off[:-1], lens) + np.arange(off[-1])
    return np.ascontiguousarray(t[idx]) if off[-1] else np.zeros(1, dtype=np.uint8), off


def expansion(data, off):
    """every context and the context plus each byte: 257 patterns per context -> (data, off)"""
    lens = np.diff(off)
    c = lens.size
    lens_e = np.repeat(lens, 257) + np.tile(np.r_[0, np.ones(256, dtype=np.int64)], c)
    off_e = np.zeros(c * 257 + 1, dtype=np.int64)
    off_e[1:] = np.cumsum(lens_e)
    pat = np.repeat(np.arange(c * 257), lens_e)
    pos = np.arange(off_e[-1]) - off_e[pat]
    ctx = pat // 257
    extra = pos == lens[ctx]
    out = np.where(extra, (pat % 257 - 1) & 0xFF, data[np.minimum(off[ctx] + pos, data.size - 1)]).astype(np.uint8)
    return np.ascontiguousarray(out), off_e


class Caller:
    def __init__(self, ix):
        self.ix, self.L = ix, sa.lib()
        self.bufs = {}

    def out(self, cnt, capacity):
        """the result arrays of a batch shape, allocated and touched once: a timed call measures the library, not the page faults"""
        key = (cnt, capacity)
        if key not in self.bufs:
            self.bufs.clear()
            self.bufs[key] = (np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32),
                              np.zeros(cnt, dtype=np.uint8), np.zeros(cnt + 1, dtype=np.int64), np.zeros(capacity, dtype=np.uint8),
                              np.zeros(capacity, dtype=np.uint32))
        return self.bufs[key]

    def search(self, data, off):
        cnt = off.size - 1
        lo, hi = np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32)
        assert self.L.sa_amd_index_search(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, None, lo.ctypes.data, hi.ctypes.data, None, None) == 0
        return lo, hi

    def next_bytes(self, data, off, capacity):
        cnt = off.size - 1
        _, lo, hi, ae, loff, b, c = self.out(cnt, capacity)
        tot = ctypes.c_int64(0)
        assert self.L.sa_amd_index_next_bytes(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, lo.ctypes.data, hi.ctypes.data, ae.ctypes.data,
                                              loff.ctypes.data, b.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot)) == 0
        assert tot.value <= capacity
        return lo, hi, ae, loff, b[:tot.value], c[:tot.value]

    def infgram(self, data, off, capacity, min_count):
        cnt = off.size - 1
        s, lo, hi, ae, loff, b, c = self.out(cnt, capacity)
        tot = ctypes.c_int64(0)
        assert self.L.sa_amd_index_infgram(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, min_count, 0, s.ctypes.data, lo.ctypes.data,
                                           hi.ctypes.data, ae.ctypes.data, loff.ctypes.data, b.ctypes.data, c.ctypes.data, capacity,
                                           ctypes.byref(tot)) == 0
        assert tot.value <= capacity
        return s, lo, hi

    def infgram_by_search(self, data, off, min_count):
        """the host loop a caller had: bisection on the suffix length, one batched search of all prompts per step"""
        lens = np.diff(off)
        cnt = lens.size
        good, bad = np.zeros(cnt, dtype=np.int64), lens + 1
        lo, hi = np.zeros(cnt, dtype=np.uint32), np.full(cnt, self.ix._s.size + 1, dtype=np.uint32)
        while True:
            live = np.flatnonzero(bad - good > 1)
            if not live.size:
                return good.astype(np.uint32), lo, hi
            s = (good[live] + bad[live]) // 2
            d, o = gather(data, off[live + 1] - s, s)
            l, h = self.search(d, o)
            ok = h.astype(np.int64) - l.astype(np.int64) >= min_count
            good[live[ok]], bad[live[~ok]] = s[ok], s[~ok]
            lo[live[ok]], hi[live[ok]] = l[ok], h[ok]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mib", type=int, default=256)
    ap.add_argument("--contexts", default="65536,1048576")
    ap.add_argument("--prompts", type=int, default=65536)
    ap.add_argument("--baseline-contexts", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--caps", default="256,1024,4096,16384")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = args.index_mib << 20
    caps = [int(c) for c in args.caps.split(",")]
    say(f"tools/ngram_bench.py: library {os.path.basename(sa.library_path())}; indexes of {args.index_mib} MiB; ms host to host, median of "
        f"{args.reps} calls after a warm-up (min..max); the 257-pattern expansion runs on the first {args.baseline_contexts} contexts of a batch, "
        f"both sides per context in us; default stream cap {sa.NGRAM_STREAM_CAP_DEFAULT}")
    beaten = True
    for label, t, held in (("English-like", corpus.english_corpus(n, 3), corpus.english_corpus(1 << 24, 5)), ("DNA", corpus.dna(n, 4), corpus.dna(1 << 24, 6))):
        ix = sa.DeviceIndex(t)
        call = Caller(ix)
        rng = np.random.default_rng(7)
        say(f"\n== {label}, {n} bytes ==")
        batches = [("256 single-byte contexts", np.arange(256, dtype=np.uint8), np.arange(257, dtype=np.int64))]
        for cnt in (int(c) for c in args.contexts.split(",")):
            lens = rng.integers(8, 33, cnt)
            batches.append((f"{cnt} contexts of 8..32 bytes", *gather(t, rng.integers(0, n - 32, cnt), lens)))
        for name, data, off in batches:
            cnt = off.size - 1
            capacity = min(256 * cnt, max(1 << 16, 16 * cnt))
            ours = timed(lambda: call.next_bytes(data, off, capacity), args.reps)
            lo, hi, ae, loff, b, c = call.next_bytes(data, off, capacity)
            st = sa.last_ngram_stats()
            sub = min(cnt, args.baseline_contexts)
            de, oe = expansion(data, off[:sub + 1])
            base = timed(lambda: call.search(de, oe), args.reps)
            el, eh = call.search(de, oe)
            el, eh = el.reshape(sub, 257), eh.reshape(sub, 257)
            dense = np.zeros((sub, 256), dtype=np.int64)
            k = int(loff[sub])
            dense[np.repeat(np.arange(sub), np.diff(loff[:sub + 1])), b[:k]] = c[:k]
            assert np.array_equal(el[:, 0], lo[:sub]) and np.array_equal(eh[:, 0], hi[:sub])
            assert np.array_equal(eh[:, 1:].astype(np.int64) - el[:, 1:], dense), "the expansion's counts differ"
            us_ours, us_base = statistics.median(ours) * 1e3 / cnt, statistics.median(base) * 1e3 / sub
            beaten &= us_ours < us_base
            say(f"{name}: next_bytes {spread(ours)} ms = {us_ours:.3f} us/context; expansion of {sub} contexts {spread(base)} ms = {us_base:.3f} us/context; "
                f"ratio {us_base / us_ours:.1f}x; entries {st['entries']}, routes stream/search/empty {st['stream_queries']}/{st['search_queries']}/"
                f"{st['empty_queries']}, slots streamed {st['stream_slots']}, probed {st['search_slots']}")
            if cnt <= 65536:
                row = []
                for cap in caps:                                      # the A/B of the stream cap
                    prev = sa.ngram_set_stream_cap(cap)
                    try:
                        row.append(f"{cap}: {spread(timed(lambda: call.next_bytes(data, off, capacity), args.reps))}")
                    finally:
                        sa.ngram_set_stream_cap(prev)
                say("   by stream cap: " + "; ".join(row))
        # ---- back-off ----
        pc = args.prompts
        held_d, held_o = gather(held, rng.integers(0, held.size - 256, pc), np.full(pc, 256))
        sl_d, sl_o = gather(t, rng.integers(0, n - 256, pc), np.full(pc, 256))
        sl_d = sl_d.copy()
        hit = rng.random(sl_d.size) < 0.01
        sl_d[hit] = rng.integers(0, 256, int(hit.sum())).astype(np.uint8)
        for name, data, off in ((f"{pc} held-out prompts of 256 bytes", held_d, held_o), (f"{pc} slices of 256 bytes, 1 % substituted", sl_d, sl_o)):
            for min_count in (1, 2):
                ours = timed(lambda: call.infgram(data, off, 256 * pc if pc < 4096 else 16 * pc, min_count), args.reps)
                s, lo, hi = call.infgram(data, off, 256 * pc if pc < 4096 else 16 * pc, min_count)
                st = sa.last_ngram_stats()
                base = timed(lambda: call.infgram_by_search(data, off, min_count), args.reps)
                bs, bl, bh = call.infgram_by_search(data, off, min_count)
                assert np.array_equal(bs, s) and np.array_equal(bl, lo) and np.array_equal(bh, hi), "the host loop's answers differ"
                mo, mb = statistics.median(ours), statistics.median(base)
                beaten &= mo < mb
                say(f"{name}, min_count {min_count}: infgram {spread(ours)} ms; host bisection over search {spread(base)} ms; ratio {mb / mo:.1f}x; "
                    f"mean s {s.mean():.1f}, range searches {st['range_searches']} ({st['range_searches'] / pc:.1f} per prompt), "
                    f"compared bytes {st['compared_bytes']}")
        ix.close()
    say(f"\nevery row faster than its baseline: {'yes' if beaten else 'NO'}")
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
