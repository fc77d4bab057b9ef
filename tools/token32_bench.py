"""DESIGN.md section 25, measured: the 32-bit token texts, ids below 2^24 (kernels/tokens.hpp), after tools/token_bench.py.

python tools/token32_bench.py [--tokens-mib 128] [--contexts 65536] [--reps 5] [--out profiles/token32_table.txt]

Build, for n tokens of corpus.token_corpus_u32(n, 128000, 3) and n uniform ids below 2^24:
  image_ms / build_ms / compact_ms of the token build (sa_amd_tok32_index_create with SA == NULL: nothing is downloaded), the
  median of --reps builds after a warm-up;
  a device-to-device copy of 16 n + 8 bytes: the bytes the compaction moves (3 n + 1 entries read, n + 1 written; its counting
  pass reads the 3 n + 1 entries once more), for the achieved bandwidth.
Widths, on the ids of corpus.token_corpus(n, 50000, 3), which fit 16 bits: the same three times from TokenIndex (2 bytes a token
  in the image) and from TokenIndex32 (3 bytes); by image bytes the expected ratio of the builds is 1.5.
Queries (the rows of section 23) on the vocabulary of 128 000: search, next_tokens and infgram for --contexts contexts of 1, 4
  and 16 tokens sampled from the text and prompts of 256 tokens (slices with 1 % of their tokens substituted), host to host.
Every figure is recorded, none is a threshold."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import suffix_array_amd as sa
from suffix_array_amd import corpus
from token_bench import Device, copy_ms, gather, result_buffers, spread, timed

PARTS = ("image_ms", "build_ms", "compact_ms")


def build_times(make_index, reps):
    """-> ({part: [ms]}, [sum ms], the last index): reps builds after a warm-up, each index closed before the next is built"""
    parts = {k: [] for k in PARTS}
    ix = None
    for rep in range(reps + 1):
        if ix is not None:
            ix.close()
        ix = make_index()
        st = sa.last_tok_stats()
        if rep:
            for k in PARTS:
                parts[k].append(st[k])
    return parts, [a + b + c for a, b, c in zip(*parts.values())], ix


def parts_line(parts, total):
    return "; ".join(f"{k} {spread(v)}" for k, v in parts.items()) + f"; sum {spread(total)}"


class Tok32Caller:
    def __init__(self, ix):
        self.ix, self.L = ix, sa.lib()

    def search(self, data, off):
        cnt = off.size - 1
        lo, hi = np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32)
        assert self.L.sa_amd_tok32_index_search(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, None, lo.ctypes.data, hi.ctypes.data) == 0
        return lo, hi

    def query(self, data, off, capacity, backoff, bufs):
        cnt = off.size - 1
        s, lo, hi, ae, loff, t, c = bufs
        tot = ctypes.c_int64(0)
        if backoff:
            rc = self.L.sa_amd_tok32_index_infgram(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, 1, 0, s.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                                   ae.ctypes.data, loff.ctypes.data, t.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot))
        else:
            rc = self.L.sa_amd_tok32_index_next_tokens(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, lo.ctypes.data, hi.ctypes.data, ae.ctypes.data,
                                                       loff.ctypes.data, t.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot))
        assert rc == 0, rc
        return int(tot.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens-mib", type=int, default=128)
    ap.add_argument("--contexts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = args.tokens_mib << 20
    cnt = args.contexts
    dev = Device()
    say(f"tools/token32_bench.py: library {os.path.basename(sa.library_path())}; texts of {n} tokens ({4 * n} bytes stored, {3 * n} bytes of image); "
        f"ms, median of {args.reps} after a warm-up (min..max); queries host to host; default stream cap {sa.NGRAM_STREAM_CAP_DEFAULT}")
    rng = np.random.default_rng(11)
    texts = (("token_corpus_u32(n, 128000, 3)", lambda: corpus.token_corpus_u32(n, 128000, 3), True),
             ("uniform ids below 2^24", lambda: np.random.default_rng(5).integers(0, 1 << 24, n, dtype=np.uint32), False))
    for label, make, with_queries in texts:
        t = np.ascontiguousarray(make(), dtype=np.uint32)
        say(f"\n== {label}: {n} tokens, {np.unique(t[:1 << 22]).size} distinct in the first 4 Mi ==")
        parts, total, ix = build_times(lambda: sa.TokenIndex32(t), args.reps)
        say("token build (index, nothing downloaded): " + parts_line(parts, total))
        moved = 16 * n + 8
        cp = copy_ms(dev, moved, args.reps)
        mc = statistics.median(cp)
        say(f"device-to-device copy of 16 n + 8 = {moved} bytes: {spread(cp)} = {2 * moved / mc / 1e6:.0f} GB/s read + written")
        cm, im = statistics.median(parts["compact_ms"]), statistics.median(parts["image_ms"])
        say(f"ratio compact_ms / copy: {cm / mc:.2f}   ({cm:.3f} ms against {mc:.3f} ms; the counting pass reads 12 n bytes more)")
        say(f"image pass: 7 n = {7 * n} bytes in {im:.3f} ms = {7 * n / im / 1e6:.0f} GB/s read + written (the range flag's read-back inside)")
        if with_queries:
            call = Tok32Caller(ix)
            capacity = 64 * cnt
            for k in (1, 4, 16):
                starts = rng.integers(0, n - 300, cnt)
                data, off = gather(t, starts, np.full(cnt, k))
                ts = timed(lambda: call.search(data, off), args.reps)
                tb = result_buffers(cnt, capacity, np.uint32)
                tn = timed(lambda: call.query(data, off, capacity, False, tb), args.reps)
                entries = call.query(data, off, capacity, False, tb)
                st = sa.last_tok_stats()
                say(f"{cnt} contexts of {k} tokens: search {spread(ts)} ms, next_tokens {spread(tn)} ms (entries {entries}, first {min(entries, capacity)} "
                    f"written; routes stream/search/empty {st['stream_queries']}/{st['search_queries']}/{st['empty_queries']}, slots streamed "
                    f"{st['stream_slots']}, probed {st['search_slots']})")
            starts = rng.integers(0, n - 300, cnt)
            data, off = gather(t, starts, np.full(cnt, 256))
            data = data.copy()
            hit = rng.random(data.size) < 0.01
            data[hit] = rng.integers(0, 1 << 24, int(hit.sum())).astype(np.uint32)
            tb = result_buffers(cnt, capacity, np.uint32)
            ti = timed(lambda: call.query(data, off, capacity, True, tb), args.reps)
            st = sa.last_tok_stats()
            say(f"{cnt} prompts of 256 tokens, 1 % substituted: infgram {spread(ti)} ms; mean s {tb[0].mean():.2f} tokens, range searches "
                f"{st['range_searches']} ({st['range_searches'] / cnt:.1f} per prompt), compared tokens {st['compared_tokens']}")
        ix.close()
        sa.lib().sa_amd_release_cache()
    # ---- the two widths on ids that fit 16 bits ----
    t16 = np.ascontiguousarray(corpus.token_corpus(n, 50000, 3), dtype=np.uint16)
    t32 = t16.astype(np.uint32)
    say(f"\n== token_corpus(n, 50000, 3), the same ids at both widths: {n} tokens ==")
    sums = {}
    for name, make in (("TokenIndex   (2 bytes a token in the image)", lambda: sa.TokenIndex(t16)),
                       ("TokenIndex32 (3 bytes a token in the image)", lambda: sa.TokenIndex32(t32))):
        parts, total, ix = build_times(make, args.reps)
        ix.close()
        sa.lib().sa_amd_release_cache()
        sums[name] = statistics.median(total)
        say(f"{name}: " + parts_line(parts, total))
    narrow, wide = sums.values()
    say(f"ratio TokenIndex32 build / TokenIndex build: {wide / narrow:.2f}   (by image bytes: 1.5)")
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
