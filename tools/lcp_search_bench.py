"""DESIGN.md section 11, measured: the LCP route of the device index's batched search (enable_lcp, kernels/esa.hpp) against the
plain route (k_search_batch), on the headline English corpus and a repetitive DNA text with planted repeats.

python tools/lcp_search_bench.py [--workloads c3_english_256m,dna_repeats_256m] [--reps 5]

Per workload: the time of enable_lcp (fresh index, array passed in: the LCP build plus the table), then for patterns of 8, 32,
1 KiB and 64 KiB bytes cut from the text (half of them with one byte changed at a random depth) one sa_amd_index_search call
per route and repetition -- host patterns in, host results out -- the two routes alternating after a warm-up call of each,
median and spread (min..max) of the repetitions.  The two routes run on two indexes of the same text and array (an index
with the table always takes the LCP route).  Every output of both routes is compared in full; compared bytes and steps per
query come from last_search_stats."""
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

M256 = 256 << 20
WORKLOADS = {
    "c3_english_256m": lambda: corpus.workload("c3_english_256m"),
    "dna_repeats_256m": lambda: corpus.dna_repeats(M256, 9, 0.4),      # (the repetitive text of the section 10 table)
}
# pattern length -> patterns per call
SHAPES = ((8, 1 << 20), (32, 1 << 20), (1 << 10, 1 << 16), (64 << 10, 1 << 10))


def patterns(rng, t, plen, cnt):
    n = t.size
    pos = rng.integers(0, n - plen, cnt)
    data = np.empty((cnt, plen), dtype=np.uint8)
    for j in range(0, plen, 4096):                                    # (gathered in column blocks: 64 KiB x 1024 is 64 MiB)
        w = min(4096, plen - j)
        data[:, j:j + w] = t[pos[:, None] + j + np.arange(w)[None, :]]
    miss = np.flatnonzero(rng.random(cnt) < 0.5)
    depth = rng.integers(0, plen, miss.size)
    data[miss, depth] ^= np.uint8(0x5A)
    off = np.arange(cnt + 1, dtype=np.int64) * plen
    return data.reshape(-1), off


def one_call(ix, data, off, out):
    c, lo, hi, ls, ll = out
    t0 = time.perf_counter()
    rc = sa.lib().sa_amd_index_search(ix._h, data.ctypes.data, off.ctypes.data, off.size - 1, c.ctypes.data, lo.ctypes.data,
                                      hi.ctypes.data, ls.ctypes.data, ll.ctypes.data)
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt


def spread(xs):
    return f"{statistics.median(xs):9.2f} ({min(xs):.2f}..{max(xs):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {sa.device_pci_bus_id(0)}; median ({args.reps} calls) and min..max; q/s = queries per second of one call "
          f"(upload, kernel, download)", flush=True)
    for name in args.workloads.split(","):
        t = WORKLOADS[name]()
        n = t.size
        plain = sa.DeviceIndex(t)
        arr = plain.suffix_array()
        en = []
        for _ in range(3):                                            # enable_lcp on a fresh index each time
            ix = sa.DeviceIndex(t, arr)
            t0 = time.perf_counter()
            ix.enable_lcp()
            en.append((time.perf_counter() - t0) * 1e3)
            ix.close()
        lcp = sa.DeviceIndex(t, arr)
        lcp.enable_lcp()
        print(f"\n== {name}: n = {n}, enable_lcp {spread(en)} ms (3 fresh indexes), table {8 * (n + 1) / 2**20:.0f} MiB",
              flush=True)
        print(f"{'plen':>6} {'patterns':>9} {'plain ms':>24} {'lcp ms':>24} {'plain Mq/s':>11} {'lcp Mq/s':>9} {'speed-up':>8} "
              f"{'cmp B/q':>9} {'bound B/q':>9} {'table steps':>11} {'hits':>6}", flush=True)
        rng = np.random.default_rng(61)
        for plen, cnt in SHAPES:
            data, off = patterns(rng, t, plen, cnt)
            outs = {k: (np.zeros(cnt, dtype=np.uint8),) + tuple(np.zeros(cnt, dtype=np.uint32) for _ in range(4))
                    for k in ("plain", "lcp")}
            one_call(plain, data, off, outs["plain"])                  # warm-up
            one_call(lcp, data, off, outs["lcp"])
            times = {"plain": [], "lcp": []}
            for _ in range(args.reps):
                times["plain"].append(one_call(plain, data, off, outs["plain"]) * 1e3)
                times["lcp"].append(one_call(lcp, data, off, outs["lcp"]) * 1e3)
                st = sa.last_search_stats()
            for a, b in zip(outs["plain"], outs["lcp"]):
                assert np.array_equal(a, b), (name, plen)
            assert st["route"] == 1 and st["patterns"] == cnt
            lp = int(np.ceil(np.log2(n + 2)))
            bound = 2 * plen + 128 * lp
            mp, ml = statistics.median(times["plain"]), statistics.median(times["lcp"])
            print(f"{plen:6d} {cnt:9d} {spread(times['plain']):>24} {spread(times['lcp']):>24} {cnt / mp / 1e3:11.3f} "
                  f"{cnt / ml / 1e3:9.3f} {mp / ml:8.2f} {st['compared_bytes'] / cnt:9.0f} {bound:9d} "
                  f"{st['table_steps'] / st['steps']:11.3f} {int(outs['lcp'][0].sum()):6d}", flush=True)
        plain.close()
        lcp.close()


if __name__ == "__main__":
    main()
