"""DESIGN.md section 16, measured: document collections over the device index (kernels/docs.hpp) against the only route there
was before -- download the suffix array, map the positions of every range to documents on the host, de-duplicate there.

python tools/docs_bench.py [--index-mib 256] [--docs 65536] [--patterns 10000] [--chunks 256,1024,4096,16384,65536] [--reps 5]
                           [--baseline-patterns 1000] [--lib libsuffix_array_amd.so] [--out profiles/docs_bench.txt]

The text is the English-like corpus of bench.py (corpus.english_corpus(n, 3)), cut into --docs equal documents.  Times are the
median of --reps calls after a warm-up, each ending in a device synchronise, with min..max; kernel times are the summed HIP
event times of the library's own profile (sa_amd_profile_begin / _end) in one more call.  Bytes are computed from the shapes:
k_doc_of over SA reads 4 and writes 4 bytes per slot (the table is cache-resident); k_doc_count reads 4 bytes per slot of every
range (the rates are those of the memory system as a whole: repeated passes can hit the Infinity Cache, see the table's legend).  --lib names another build of the library (for the A/B of DOC_SAMPLES, which is a compile-time constant)."""
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
from suffix_array_amd import corpus

HBM_PEAK = 8.0e12          # bytes/s, the specification's figure


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


def kernel_split(fn):
    L = sa.lib()
    names = []
    while L.sa_amd_profile_kernel_name(len(names)):
        names.append(L.sa_amd_profile_kernel_name(len(names)).decode())
    L.sa_amd_profile_begin()
    fn()
    ms, launches, units = (ctypes.c_double * 32)(), (ctypes.c_int64 * 32)(), (ctypes.c_int64 * 32)()
    cnt = L.sa_amd_profile_end(ms, launches, units, 32)
    return {names[i]: (round(ms[i], 3), launches[i]) for i in range(cnt) if launches[i]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mib", type=int, default=256)
    ap.add_argument("--docs", type=int, default=65536)
    ap.add_argument("--patterns", type=int, default=10000)
    ap.add_argument("--baseline-patterns", type=int, default=1000)
    ap.add_argument("--chunks", default="256,1024,4096,16384,65536")
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
    say(f"tools/docs_bench.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(sa.library_path())}; English-like text of {args.index_mib} MiB in "
        f"{args.docs} equal documents; DOC_SAMPLES as built; ms, median of {args.reps} calls after a warm-up (min..max)")
    ix = sa.DeviceIndex(t)
    arr = ix.suffix_array()

    # ---- set_documents, and k_doc_of over the suffix array on its own ----
    sd = timed(lambda: ix.set_documents(off), args.reps)
    split = kernel_split(lambda: ix.set_documents(off))
    say(f"\nset_documents: {spread(sd)} ms; kernel classes (ms, launches): {split}")
    say(f"   scratch {sa.docs_work_bytes(n) / 2**30:.2f} GiB from the pool; kept: {4 * (n + 1) / 2**30:.2f} GiB + the offsets")
    dSA = torch.from_numpy(arr.view(np.int32)).cuda()
    dOut = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    do = timed(lambda: sa.doc_of_device_ptr(ix, dSA.data_ptr(), n + 1, dOut.data_ptr()), args.reps)
    rate = 8.0 * (n + 1) / (statistics.median(do) * 1e-3)
    say(f"k_doc_of over SA (random positions, device pointers): {spread(do)} ms = {rate / 1e9:.0f} GB/s of 4 + 4 bytes per slot = "
        f"{100 * rate / HBM_PEAK:.1f} % of the HBM peak")
    assert np.array_equal(dOut.cpu().numpy().view(np.uint32)[1:1 << 20], (np.searchsorted(off, arr[1:1 << 20], "right") - 1).astype(np.uint32))
    del dSA, dOut
    say(f"   derived, not measured apart: k_doc_prev = the misc class of set_documents ({split['misc'][0]:.3f} ms, k_doc_of over SA[1..n] + k_doc_prev) "
        f"less k_doc_of over SA above = {split['misc'][0] - statistics.median(do):.1f} ms")
    rnd = np.random.default_rng(1).integers(0, n, 1 << 24).astype(np.uint32)
    say(f"doc_of, host pointers, {rnd.size} random positions: {spread(timed(lambda: ix.doc_of(rnd), args.reps))} ms")

    # ---- k_doc_count as a stream: the empty pattern's range is every slot ----
    say(f"\nstream columns: kernel time = HIP events of all six kernels of the call (five of them a few microseconds); 16 x = sixteen "
        f"passes over the same {4 * (n + 1) / 2**30:.2f} GiB of words, of which the 256 MiB Infinity Cache can serve a part; 1 x = one pass, a "
        f"window of well under a millisecond")
    say(f"{'chunk':>7} {'16 x empty pattern, call ms':>32} {'16 x GB/s':>10} {'% peak':>6} {'1 x kernels ms':>15} {'1 x GB/s':>9} {'% peak':>6}   |   "
        f"{args.patterns} patterns of 4-16 bytes: {'doc_search ms':>26} {'doc_list ms':>26} {'units':>9}")
    rng = np.random.default_rng(2)
    starts = rng.integers(0, n - 16, args.patterns)
    pats = [tb[int(a):int(a) + int(k)] for a, k in zip(starts, rng.integers(4, 17, args.patterns))]
    data, poff, cnt = sa._pattern_batch(pats)
    L = sa.lib()
    occ, df = ix.doc_search(pats)
    total = int(df.sum())
    loff = np.zeros(cnt + 1, dtype=np.int64)
    docs = np.empty(total + 1, dtype=np.uint32)
    tot = ctypes.c_int64(0)

    def search():
        assert L.sa_amd_index_doc_search(ix._h, data.ctypes.data, poff.ctypes.data, cnt, occ.ctypes.data, df.ctypes.data) == 0

    def listing():
        assert L.sa_amd_index_doc_list(ix._h, data.ctypes.data, poff.ctypes.data, cnt, loff.ctypes.data, docs.ctypes.data, total + 1,
                                       ctypes.byref(tot)) == 0
    empties = [b""] * 16
    for chunk in [int(c) for c in args.chunks.split(",")]:
        sa.docs_set_chunk(chunk)
        e = timed(lambda: ix.doc_search(empties), args.reps)
        ek = kernel_split(lambda: ix.doc_search(empties))["misc"][0]
        bw = 16 * 4.0 * (n + 1) / (ek * 1e-3)
        ix.doc_search([b""])
        e1 = statistics.median([kernel_split(lambda: ix.doc_search([b""]))["misc"][0] for _ in range(args.reps)])
        bw1 = 4.0 * (n + 1) / (e1 * 1e-3)
        s, l = timed(search, args.reps), timed(listing, args.reps)
        st = sa.last_docs_stats()
        say(f"{chunk:7d} {spread(e):>32} {bw / 1e9:10.0f} {100 * bw / HBM_PEAK:6.1f} {e1:15.3f} {bw1 / 1e9:9.0f} {100 * bw1 / HBM_PEAK:6.1f}   |   {'':>{len(str(args.patterns)) + 26}} {spread(s):>26} {spread(l):>26} "
            f"{st['units']:9d}")
    sa.docs_set_chunk(-1)
    d_ms = statistics.median(timed(search, args.reps))
    l_ms = statistics.median(timed(listing, args.reps))
    sk = kernel_split(search)
    say(f"\ndefault chunk {sa.last_docs_stats()['chunk']}: occ_sum {int(occ.sum())}, df_sum {total}; doc_search {cnt / d_ms * 1e3:.0f} patterns/s, "
        f"doc_list {cnt / l_ms * 1e3:.0f} patterns/s")
    say(f"   kernels of one doc_search call (search kernel, units, k_doc_count; ms, launches): {sk}; 4 occ_sum bytes over that: "
        f"{4.0 * occ.sum() / (sk['misc'][0] * 1e-3) / 1e9:.1f} GB/s")

    # ---- the yardstick: download the array, searchsorted + unique on the host ----
    nb = min(args.baseline_patterns, cnt)
    res = ix.search(pats[:nb])
    t0 = time.perf_counter()
    full = ix.suffix_array()
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    base = [np.unique(np.searchsorted(off, full[int(a):int(b)], "right") - 1).size for a, b in zip(res["lo"], res["hi"])]
    t_host = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(np.array(base), df[:nb])
    say(f"yardstick, the first {nb} patterns: sa_amd_index_sa (whole array, {4 * (n + 1) / 2**30:.2f} GiB) {t_down:.0f} ms + np.unique(np.searchsorted) "
        f"{t_host:.1f} ms = {nb / (t_host * 1e-3):.0f} patterns/s on the host once the array is down; answers equal")
    ix.close()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
