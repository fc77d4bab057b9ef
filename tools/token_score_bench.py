"""DESIGN.md section 24, measured: TokenIndex.infgram_score (kernels/score.hpp instantiated for 16-bit tokens) beside
DeviceIndex.infgram_score on a byte index over the big-endian image of the same text, scoring the image of the same query: twice
the positions and twice the context bytes, without tables and with both (bucket table and LCP table).

python tools/token_score_bench.py [--tokens-mib 128] [--query-mib 1] [--max-lens 64,4096] [--reps 5] [--out profiles/token_score_table.txt]

Texts: corpus.token_corpus(n, 50000, 3) (Zipf) and n uniform tokens, as tools/token_bench.py.  Queries: a slice of the text with
1 % of its tokens substituted, and a foreign query (the same generator, another seed).  Times are host to host (query up, six
arrays down into arrays allocated once), ms, the median of --reps calls after a warm-up with min..max.  The byte side's max_len is
2 max_len bytes, clamped to SA_AMD_SCORE_MAX_CONTEXT = 4096 bytes (2 048 tokens' worth): the byte form cannot look further back.
The ratios are reported, not gated."""
import argparse
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


class Caller:
    """one index and the six result arrays of a query length, allocated and touched once"""

    def __init__(self, ix, entry):
        self.ix, self.entry = ix, entry
        self.bufs = {}

    def score(self, q, max_len):
        if q.size not in self.bufs:
            self.bufs.clear()
            self.bufs[q.size] = {k: np.zeros(q.size, dtype=np.uint8 if k == "at_end" else np.uint32) for k in NAMES}
        o = self.bufs[q.size]
        assert self.entry(self.ix._h, q.ctypes.data, q.size, None, 0, 1, max_len, *(o[k].ctypes.data for k in NAMES)) == 0
        return o


def counters(st, m, compared):
    return (f"mean S {st['mean_s']:.1f}, searches/pos {st['range_searches'] / m:.2f} (group {st['group_searches'] / m:.2f}, long "
            f"{st['long_searches'] / m:.2f}), long positions {st['long_positions']}, p = 0 at {st['zero_positions']}, next look-ups/pos "
            f"{st['next_lookups'] / m:.1f}, {compared.replace('_', ' ')}/pos {st[compared] / m:.0f}, group cap {st['group_cap']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens-mib", type=int, default=128)
    ap.add_argument("--query-mib", type=int, default=1)
    ap.add_argument("--max-lens", default="64,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n, m = args.tokens_mib << 20, args.query_mib << 20
    max_lens = [int(x) for x in args.max_lens.split(",")]
    L = sa.lib()
    say(f"tools/token_score_bench.py: library {os.path.basename(sa.library_path())}; texts of {n} tokens ({2 * n} bytes of image); queries of {m} "
        f"tokens ({2 * m} bytes of image), min_count 1; host to host, ms, median of {args.reps} after a warm-up (min..max); default group cap "
        f"{sa.SCORE_GROUP_CAP_DEFAULT}, 8 lanes a position")
    texts = (("token_corpus(n, 50000, 3)", lambda k, seed: corpus.token_corpus(k, 50000, seed), 3, 5),
             ("uniform tokens", lambda k, seed: np.random.default_rng(seed).integers(0, 65536, k, dtype=np.uint16), 5, 6))
    for label, make, seed, other in texts:
        t = np.ascontiguousarray(make(n, seed), dtype=np.uint16)
        image = t.astype(">u2").view(np.uint8)
        rng = np.random.default_rng(7)
        a = int(rng.integers(0, n - m))
        sl = t[a:a + m].copy()
        hit = rng.random(m) < 0.01
        sl[hit] = rng.integers(0, 65536, int(hit.sum())).astype(np.uint16)
        queries = ((f"slice of {m} tokens, 1 % substituted", sl), (f"foreign query of {m} tokens", np.ascontiguousarray(make(m, other), dtype=np.uint16)))
        tix = sa.TokenIndex(t)
        bix = sa.DeviceIndex(image)
        tok, byt = Caller(tix, L.sa_amd_tok_index_infgram_score), Caller(bix, L.sa_amd_index_infgram_score)
        rows = {}
        say(f"\n== {label}: {n} tokens ==")
        for tables in ("no tables", "bucket table and LCP table"):
            if tables != "no tables":
                bix.buckets()
                bix.enable_lcp()
            for qname, q in queries:
                qimg = np.ascontiguousarray(q.astype(">u2").view(np.uint8))
                for max_len in max_lens:
                    if tables == "no tables":
                        ms = timed(lambda: tok.score(q, max_len), args.reps)
                        st = sa.last_tok_score_stats()
                        st["mean_s"] = float(tok.score(q, max_len)["s"].mean())
                        rows[(qname, max_len, "token")] = (ms, f"token index, max_len {max_len} tokens: {spread(ms)} ms; " + counters(st, m, "compared_tokens"))
                    blen = min(2 * max_len, sa.SCORE_MAX_CONTEXT)
                    ms = timed(lambda: byt.score(qimg, blen), args.reps)
                    st = sa.last_score_stats()
                    st["mean_s"] = float(byt.score(qimg, blen)["s"].mean())
                    rows[(qname, max_len, tables)] = (ms, f"byte index on the image, {tables}, {2 * m} positions, max_len {blen} bytes: {spread(ms)} ms; "
                                                          + counters(st, 2 * m, "compared_bytes"))
        for qname, _ in queries:
            for max_len in max_lens:
                say(f"{qname}, max_len {max_len}:")
                tms = statistics.median(rows[(qname, max_len, "token")][0])
                for kind in ("token", "no tables", "bucket table and LCP table"):
                    ms, line = rows[(qname, max_len, kind)]
                    ratio = "" if kind == "token" else f"; token / byte = {tms / statistics.median(ms):.2f}"
                    say("    " + line + ratio)
        tix.close()
        bix.close()
        L.sa_amd_release_cache()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
