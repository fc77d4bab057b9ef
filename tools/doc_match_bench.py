"""DESIGN.md section 26, measured: Boolean document queries on the device (kernels/doc_match.hpp) beside the only route there
was before -- doc_list of both patterns, the listings down to the host, np.intersect1d (np.setdiff1d for NOT) there.

python tools/doc_match_bench.py [--index-mib 256] [--docs 65536] [--queries 10000] [--baseline-queries 1000] [--reps 5]
                                [--lib libsuffix_array_amd.so] [--out profiles/doc_match_table.txt]

The text is the English-like corpus of bench.py (corpus.english_corpus(n, 3)), cut into --docs equal documents.  Times are the
median of --reps calls after a warm-up, each ending in a device synchronise, with min..max; kernel times are the summed HIP event
times of the library's own profile (sa_amd_profile_begin / _end) in one more call -- every kernel of a call is of the class
"misc", so the combine pass is timed apart by a batch of the same shape whose clauses hold no patterns: no search, no units, no
marks, only the zeroing (a memset, not in the profile) and k_dm_combine over the same number of clause words."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import suffix_array_amd as sa
from suffix_array_amd import Not, corpus


def spread(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}..{max(xs):.3f})"


def timed(fn, reps):
    fn()                                                              # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_ms(fn):
    L = sa.lib()
    names = []
    while L.sa_amd_profile_kernel_name(len(names)):
        names.append(L.sa_amd_profile_kernel_name(len(names)).decode())
    L.sa_amd_profile_begin()
    fn()
    ms, launches, units = (ctypes.c_double * 32)(), (ctypes.c_int64 * 32)(), (ctypes.c_int64 * 32)()
    cnt = L.sa_amd_profile_end(ms, launches, units, 32)
    got = {names[i]: (round(ms[i], 3), launches[i]) for i in range(cnt) if launches[i]}
    assert set(got) <= {"misc"}, got
    return got.get("misc", (0.0, 0))


class Batch:
    """a packed batch of queries and the two raw calls on it"""

    def __init__(self, ix, queries):
        self.ix = ix
        self.data, self.off, self.npat, self.coff, self.cfl, self.ncl, self.qoff, self.nq = sa._query_batch(queries)
        self.df = np.zeros(self.nq, dtype=np.uint32)
        self.loff = np.zeros(self.nq + 1, dtype=np.int64)
        self.total = ctypes.c_int64(0)
        self.docs = np.zeros(1, dtype=np.uint32)

    def _inputs(self):
        return (self.ix._h, self.data.ctypes.data, self.off.ctypes.data, self.npat, self.coff.ctypes.data, self.cfl.ctypes.data, self.ncl,
                self.qoff.ctypes.data, self.nq)

    def count(self):
        assert sa.lib().sa_amd_index_doc_match(*self._inputs(), self.df.ctypes.data, None) == 0

    def listing(self):
        assert sa.lib().sa_amd_index_doc_match_list(*self._inputs(), self.loff.ctypes.data, self.docs.ctypes.data, self.docs.size,
                                                    ctypes.byref(self.total)) == 0

    def size_listing(self):
        self.count()
        self.docs = np.zeros(int(self.df.sum()) + 1, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mib", type=int, default=256)
    ap.add_argument("--docs", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--baseline-queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.lib:
        sa._LIB_NAME = args.lib                                       # (before the first call: the library is loaded once)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = args.index_mib << 20
    t = corpus.english_corpus(n, 3)
    tb = t.tobytes()
    off = (np.arange(args.docs + 1, dtype=np.int64) * n) // args.docs
    W = (args.docs + 31) // 32
    say(f"tools/doc_match_bench.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(sa.library_path())}; English-like text of {args.index_mib} MiB in {args.docs} equal documents "
        f"(W = {W} words, {4 * W} bytes of bitmap a clause); ms, median of {args.reps} calls after a warm-up (min..max)")
    ix = sa.DeviceIndex(t)
    ix.set_documents(off)
    rng = np.random.default_rng(2)
    starts = rng.integers(0, n - 16, 2 * args.queries)
    pats = [tb[int(a):int(a) + int(k)] for a, k in zip(starts, rng.integers(4, 17, 2 * args.queries))]
    first, second = pats[:args.queries], pats[args.queries:]
    sixteen = [[pats[k]] if k % 4 else Not(pats[k]) for k in range(16)]
    cases = [("two-clause AND", [[a, b] for a, b in zip(first, second)]),
             ("two-clause AND NOT", [[a, Not(b)] for a, b in zip(first, second)]),
             ("one query of sixteen clauses", [sixteen])]
    say(f"\n{'case':<30} {'queries':>8} {'doc_match ms':>28} {'kernels ms (launches)':>22} {'marks':>10} {'units':>8} {'occ_sum':>11} {'df_sum':>10} {'slabs':>5}")
    batches = {}
    for name, queries in cases:
        b = batches[name] = Batch(ix, queries)
        ms = timed(b.count, args.reps)
        k = kernel_ms(b.count)
        st = sa.last_doc_match_stats()
        say(f"{name:<30} {b.nq:8d} {spread(ms):>28} {k[0]:14.3f} ({k[1]:5d}) {st['marks']:10d} {st['units']:8d} {st['occ_sum']:11d} {st['df_sum']:10d} "
            f"{st['slabs']:5d}")
    b = batches["two-clause AND"]
    b.size_listing()
    ms = timed(b.listing, args.reps)
    k = kernel_ms(b.listing)
    st = sa.last_doc_match_stats()
    say(f"{'doc_match_list, two-clause AND':<30} {b.nq:8d} {spread(ms):>28} {k[0]:14.3f} ({k[1]:5d}) {st['marks']:10d} {st['units']:8d} {st['occ_sum']:11d} "
        f"{st['df_sum']:10d} {st['slabs']:5d}")
    assert int(b.total.value) == int(b.df.sum()) == int(b.loff[-1])

    # ---- the combine pass on its own: the same number of clause words, no patterns ----
    hollow = Batch(ix, [[[], Not([])] for _ in range(args.queries)])
    hollow.count()
    assert np.all(hollow.df == 0) and sa.last_doc_match_stats()["marks"] == 0
    km = statistics.median([kernel_ms(hollow.count)[0] for _ in range(args.reps)])
    nbytes = 4.0 * W * hollow.ncl
    say(f"\ncombine pass alone ({hollow.nq} queries of two clauses without patterns: k_dm_combine only): {km:.3f} ms kernel time over "
        f"{nbytes / 2**20:.0f} MiB = 4 W bytes per clause: {nbytes / (km * 1e-3) / 1e9:.0f} GB/s; the call: {spread(timed(hollow.count, args.reps))} ms")

    # ---- the yardstick: doc_list of both patterns, the listings down, set algebra on the host ----
    nb = min(args.baseline_queries, args.queries)
    both = first[:nb] + second[:nb]
    data, poff, cnt = sa._pattern_batch(both)
    _, dfp = ix.doc_search(both)
    cap = int(dfp.sum()) + 1
    loff = np.zeros(cnt + 1, dtype=np.int64)
    docs = np.empty(cap, dtype=np.uint32)
    tot = ctypes.c_int64(0)

    def listings():
        assert sa.lib().sa_amd_index_doc_list(ix._h, data.ctypes.data, poff.ctypes.data, cnt, loff.ctypes.data, docs.ctypes.data, cap, ctypes.byref(tot)) == 0
    dl = timed(listings, args.reps)
    for name, op in (("two-clause AND", np.intersect1d), ("two-clause AND NOT", np.setdiff1d)):
        host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sizes = [op(docs[loff[q]:loff[q + 1]], docs[loff[nb + q]:loff[nb + q + 1]]).size for q in range(nb)]
            host.append((time.perf_counter() - t0) * 1e3)
        small = Batch(ix, [[a, Not(b)] if op is np.setdiff1d else [a, b] for a, b in zip(first[:nb], second[:nb])])
        dev = timed(small.count, args.reps)
        assert np.array_equal(np.array(sizes, dtype=np.uint32), small.df)
        say(f"yardstick, the first {nb} queries, {name}: doc_list of {cnt} patterns {spread(dl)} ms ({4 * (cap - 1) / 2**20:.1f} MiB of listing down) + "
            f"{op.__name__} on the host {spread(host)} ms; doc_match of the same {nb} queries {spread(dev)} ms; answers equal")
    ix.close()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
