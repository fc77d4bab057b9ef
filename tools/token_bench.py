"""DESIGN.md section 23, measured: the 16-bit token texts (kernels/tokens.hpp).

python tools/token_bench.py [--tokens-mib 128] [--contexts 65536] [--reps 5] [--out profiles/token_table.txt]

Build, for n tokens of corpus.token_corpus(n, 50000, 3) and n uniform tokens:
  image_ms / build_ms / compact_ms of the token build (sa_amd_tok_index_create with SA == NULL: nothing is downloaded), the
  median of --reps builds after a warm-up;
  sa_amd_saca_device on the same 2 n-byte big-endian image in the same process: the yardstick, the byte builder alone;
  sa_amd_saca_device on the first n bytes of that image: a byte text with as many symbols as the token text has tokens -- what a
  native token key builder (n suffixes sorted instead of 2 n) could at best approach;
  a device-to-device copy of 12 n + 4 bytes: the bytes the compaction moves (2 n + 1 entries read, n + 1 written; its counting
  pass reads the 2 n + 1 entries once more), for the achieved bandwidth.
  Ratios: (image_ms + compact_ms) / copy, token build / byte build of n bytes.  No ratio is a threshold.
Queries: search, next_tokens and infgram for --contexts contexts of 1, 4 and 16 tokens sampled from the text and prompts of 256
  tokens (slices with 1 % of their tokens substituted), host to host, beside sa_amd_index_search / next_bytes / infgram on a
  byte index over the image (the same bytes) with contexts of 2, 8 and 32 bytes and prompts of 512 bytes."""
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

H2D, D2D = 1, 3


def spread(xs):
    return f"{statistics.median(xs):10.3f} ({min(xs):.3f}..{max(xs):.3f})"


def timed(fn, reps):
    out = []
    for _ in range(reps + 1):                                         # (the first call is the warm-up; every call blocks until done)
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def hip_runtime():
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    return hip


class Device:
    def __init__(self):
        self.hip = hip_runtime()
        self.held = []

    def malloc(self, size):
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), max(int(size), 1)) == 0, f"hipMalloc({size})"
        self.held.append(p.value)
        return p.value

    def free_all(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


def gather(t, starts, lens):
    """the batch of t[starts[q] : starts[q] + lens[q]] -> (data, off)"""
    off = np.zeros(starts.size + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    idx = np.repeat(starts - off[:-1], lens) + np.arange(off[-1])
    return np.ascontiguousarray(t[idx]), off


class TokCaller:
    def __init__(self, ix):
        self.ix, self.L = ix, sa.lib()

    def search(self, data, off):
        cnt = off.size - 1
        lo, hi = np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32)
        assert self.L.sa_amd_tok_index_search(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, None, lo.ctypes.data, hi.ctypes.data) == 0
        return lo, hi

    def query(self, data, off, capacity, backoff, bufs):
        cnt = off.size - 1
        s, lo, hi, ae, loff, t, c = bufs
        tot = ctypes.c_int64(0)
        if backoff:
            rc = self.L.sa_amd_tok_index_infgram(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, 1, 0, s.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                                 ae.ctypes.data, loff.ctypes.data, t.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot))
        else:
            rc = self.L.sa_amd_tok_index_next_tokens(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, lo.ctypes.data, hi.ctypes.data, ae.ctypes.data,
                                                     loff.ctypes.data, t.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot))
        assert rc == 0, rc
        return int(tot.value)


class ByteCaller:
    def __init__(self, ix):
        self.ix, self.L = ix, sa.lib()

    def search(self, data, off):
        cnt = off.size - 1
        lo, hi = np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32)
        assert self.L.sa_amd_index_search(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, None, lo.ctypes.data, hi.ctypes.data, None, None) == 0
        return lo, hi

    def query(self, data, off, capacity, backoff, bufs):
        cnt = off.size - 1
        s, lo, hi, ae, loff, t, c = bufs
        tot = ctypes.c_int64(0)
        if backoff:
            rc = self.L.sa_amd_index_infgram(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, 1, 0, s.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                             ae.ctypes.data, loff.ctypes.data, t.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot))
        else:
            rc = self.L.sa_amd_index_next_bytes(self.ix._h, data.ctypes.data, off.ctypes.data, cnt, lo.ctypes.data, hi.ctypes.data, ae.ctypes.data,
                                                loff.ctypes.data, t.ctypes.data, c.ctypes.data, capacity, ctypes.byref(tot))
        assert rc == 0, rc
        return int(tot.value)


def result_buffers(cnt, capacity, unit):
    return (np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint32), np.zeros(cnt, dtype=np.uint8),
            np.zeros(cnt + 1, dtype=np.int64), np.zeros(capacity, dtype=unit), np.zeros(capacity, dtype=np.uint32))


def byte_build_ms(dev, image, nbytes, reps):
    """sa_amd_saca_device on image[:nbytes], device buffers of the tool's own; ms of the blocking call"""
    wb = sa.workspace_bytes(nbytes)
    d_t, d_sa, d_w = dev.malloc(nbytes + 16), dev.malloc(4 * (nbytes + 1)), dev.malloc(wb)
    assert dev.hip.hipMemcpy(d_t, image.ctypes.data, nbytes, H2D) == 0
    ms = timed(lambda: sa.saca_device_ptr(d_t, d_sa, nbytes, d_w, wb), reps)
    dev.free_all()
    return ms


def copy_ms(dev, nbytes, reps):
    a, b = dev.malloc(nbytes), dev.malloc(nbytes)

    def run():
        assert dev.hip.hipMemcpy(b, a, nbytes, D2D) == 0
        assert dev.hip.hipDeviceSynchronize() == 0
    ms = timed(run, reps)
    dev.free_all()
    return ms


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
    say(f"tools/token_bench.py: library {os.path.basename(sa.library_path())}; texts of {n} tokens ({2 * n} bytes of image); ms, median of {args.reps} "
        f"after a warm-up (min..max); queries host to host; default stream cap {sa.NGRAM_STREAM_CAP_DEFAULT}")
    rng = np.random.default_rng(11)
    texts = (("token_corpus(n, 50000, 3)", lambda: corpus.token_corpus(n, 50000, 3)),
             ("uniform tokens", lambda: np.random.default_rng(5).integers(0, 65536, n, dtype=np.uint16)))
    for label, make in texts:
        t = np.ascontiguousarray(make(), dtype=np.uint16)
        image = t.astype(">u2").view(np.uint8)
        say(f"\n== {label}: {n} tokens, {np.unique(t[:1 << 22]).size} distinct in the first 4 Mi ==")
        # ---- build ----
        parts = {"image_ms": [], "build_ms": [], "compact_ms": []}
        ix = None
        for rep in range(args.reps + 1):
            if ix is not None:
                ix.close()
            ix = sa.TokenIndex(t)
            st = sa.last_tok_stats()
            if rep:
                for k in parts:
                    parts[k].append(st[k])
        total = [a + b + c for a, b, c in zip(*parts.values())]
        say("token build (index, nothing downloaded): " + "; ".join(f"{k} {spread(v)}" for k, v in parts.items()) + f"; sum {spread(total)}")
        same_image = byte_build_ms(dev, image, 2 * n, args.reps)
        say(f"sa_amd_saca_device on the same image ({2 * n} bytes): {spread(same_image)}")
        half = byte_build_ms(dev, image, n, args.reps)
        say(f"sa_amd_saca_device on {n} bytes (the first half of the image): {spread(half)}")
        moved = 12 * n + 4
        cp = copy_ms(dev, moved, args.reps)
        mc = statistics.median(cp)
        say(f"device-to-device copy of 12 n + 4 = {moved} bytes: {spread(cp)} = {2 * moved / mc / 1e6:.0f} GB/s read + written")
        stream = statistics.median(parts["image_ms"]) + statistics.median(parts["compact_ms"])
        say(f"ratio (image_ms + compact_ms) / copy: {stream / mc:.2f}   ({stream:.3f} ms against {mc:.3f} ms; the image pass moves 4 n bytes more)")
        say(f"ratio token build / byte build of n bytes: {statistics.median(total) / statistics.median(half):.2f}   "
            f"(token build / byte build of the same image: {statistics.median(total) / statistics.median(same_image):.3f})")
        # ---- queries ----
        tok_call = TokCaller(ix)
        bix = sa.DeviceIndex(image)
        byte_call = ByteCaller(bix)
        capacity = 64 * cnt
        for k in (1, 4, 16):
            starts = rng.integers(0, n - 300, cnt)
            data, off = gather(t, starts, np.full(cnt, k))
            bdata, boff = gather(image, 2 * starts, np.full(cnt, 2 * k))
            ts = timed(lambda: tok_call.search(data, off), args.reps)
            bs = timed(lambda: byte_call.search(bdata, boff), args.reps)
            tb, bb = result_buffers(cnt, capacity, np.uint16), result_buffers(cnt, capacity, np.uint8)
            tn = timed(lambda: tok_call.query(data, off, capacity, False, tb), args.reps)
            entries = tok_call.query(data, off, capacity, False, tb)
            st = sa.last_tok_stats()
            bn = timed(lambda: byte_call.query(bdata, boff, capacity, False, bb), args.reps)
            say(f"{cnt} contexts of {k} tokens: search {spread(ts)} ms, next_tokens {spread(tn)} ms (entries {entries}, first {min(entries, capacity)} "
                f"written; routes stream/search/empty {st['stream_queries']}/{st['search_queries']}/{st['empty_queries']}, slots streamed "
                f"{st['stream_slots']}, probed {st['search_slots']})")
            say(f"    byte index, contexts of {2 * k} bytes: search {spread(bs)} ms, next_bytes {spread(bn)} ms")
        starts = rng.integers(0, n - 300, cnt)
        data, off = gather(t, starts, np.full(cnt, 256))
        data = data.copy()
        hit = rng.random(data.size) < 0.01
        data[hit] = rng.integers(0, 65536, int(hit.sum())).astype(np.uint16)
        bdata = np.ascontiguousarray(data.astype(">u2").view(np.uint8))
        boff = 2 * off
        tb, bb = result_buffers(cnt, capacity, np.uint16), result_buffers(cnt, capacity, np.uint8)
        ti = timed(lambda: tok_call.query(data, off, capacity, True, tb), args.reps)
        st = sa.last_tok_stats()
        bi = timed(lambda: byte_call.query(bdata, boff, capacity, True, bb), args.reps)
        bst = sa.last_ngram_stats()
        say(f"{cnt} prompts of 256 tokens, 1 % substituted: infgram {spread(ti)} ms; mean s {tb[0].mean():.2f} tokens, range searches "
            f"{st['range_searches']} ({st['range_searches'] / cnt:.1f} per prompt), compared tokens {st['compared_tokens']}")
        say(f"    byte index, prompts of 512 bytes: infgram {spread(bi)} ms; mean s {bb[0].mean():.2f} bytes, range searches "
            f"{bst['range_searches']} ({bst['range_searches'] / cnt:.1f} per prompt)")
        ix.close()
        bix.close()
        sa.lib().sa_amd_release_cache()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
