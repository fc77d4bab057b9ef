"""DESIGN.md section 18, measured: per-document term frequencies and top-k documents over the device index (kernels/doc_tf.hpp)
beside the listing they extend -- doc_list on the same index, the same batches, in the same process is the yardstick.

python tools/doc_tf_bench.py [--index-mib 256] [--docs 65536] [--words 4096] [--grams 65536] [--k 10] [--pieces 1024,2048,4096]
                             [--reps 3] [--lib libsuffix_array_amd_diag.so] [--out profiles/doc_tf_bench.txt]

The text is the English-like corpus of bench.py (corpus.english_corpus(n, 3)), cut into --docs equal documents.  Batches: 16 x the
empty pattern (every slot, every document), the --words most common words of the text's first 4 MiB, --grams random 8-grams of
the text.  Times are the median of --reps calls after a warm-up, each ending in a device synchronise, with min..max; they include
the copies of the results to the host, as a caller sees them.  The A/B of the second bound of k_doc_tf (galloping against a plain
binary search) needs the diagnostic library's switch: it runs when --lib names that library."""
import argparse
import collections
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


def spread(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}..{max(xs):.3f})"


def timed(fn, reps, before=None):
    out = []
    for i in range(reps + 1):                                         # (the first call is the warm-up)
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def kernel_ms(fn):
    L = sa.lib()
    names = []
    while L.sa_amd_profile_kernel_name(len(names)):
        names.append(L.sa_amd_profile_kernel_name(len(names)).decode())
    L.sa_amd_profile_begin()
    fn()
    ms, launches, units = (ctypes.c_double * 32)(), (ctypes.c_int64 * 32)(), (ctypes.c_int64 * 32)()
    cnt = L.sa_amd_profile_end(ms, launches, units, 32)
    return sum(ms[i] for i in range(cnt)), sum(launches[i] for i in range(cnt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-mib", type=int, default=256)
    ap.add_argument("--docs", type=int, default=65536)
    ap.add_argument("--words", type=int, default=4096)
    ap.add_argument("--grams", type=int, default=65536)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pieces", default="1024,2048,4096")
    ap.add_argument("--reps", type=int, default=3)
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
    L = sa.lib()
    say(f"tools/doc_tf_bench.py: {torch.cuda.get_device_name(0)}, library {os.path.basename(sa.library_path())}; English-like text of {args.index_mib} MiB in "
        f"{args.docs} equal documents; k = {args.k}; ms, median of {args.reps} calls after a warm-up (min..max), results copied to the host")
    ix = sa.DeviceIndex(t)

    # ---- the tables ----
    sd = timed(lambda: ix.set_documents(off), args.reps)
    en = timed(ix.enable_doc_freq, args.reps, before=lambda: ix.set_documents(off))
    ix.set_documents(off)
    say(f"\nset_documents {spread(sd)} ms; enable_doc_freq {spread(en)} ms (kernels {kernel_ms(ix.enable_doc_freq)[0]:.3f} ms); the table keeps "
        f"{4 * n / 2**30:.2f} GiB beside the collection's {4 * (n + 1) / 2**30:.2f} GiB")
    ix.enable_doc_freq()

    # ---- the batches ----
    rng = np.random.default_rng(2)
    words = [w for w, _ in collections.Counter(tb[:4 << 20].split()).most_common(args.words)]
    words = (words * (args.words // max(len(words), 1) + 1))[:args.words]
    starts = rng.integers(0, n - 8, args.grams)
    batches = [("16 x empty pattern", [b""] * 16), (f"{len(words)} common words", words),
               (f"{args.grams} random 8-grams", [tb[int(a):int(a) + 8] for a in starts])]
    can_ab = hasattr(ctypes.CDLL(sa.library_path()), "sa_amd_debug_doc_tf_bounds")
    pieces = [int(p) for p in args.pieces.split(",")]
    for name, pats in batches:
        data, poff, cnt = sa._pattern_batch(pats)
        occ, df = ix.doc_search(pats)
        total = int(df.sum())
        loff = np.zeros(cnt + 1, dtype=np.int64)
        docs = np.empty(total + 1, dtype=np.uint32)
        tf = np.empty(total + 1, dtype=np.uint32)
        tdocs = np.empty(cnt * args.k + 1, dtype=np.uint32)
        ttf = np.empty(cnt * args.k + 1, dtype=np.uint32)
        tot = ctypes.c_int64(0)

        def listing():
            assert L.sa_amd_index_doc_list(ix._h, data.ctypes.data, poff.ctypes.data, cnt, loff.ctypes.data, docs.ctypes.data, total + 1,
                                           ctypes.byref(tot)) == 0

        def freq():
            assert L.sa_amd_index_doc_tf(ix._h, data.ctypes.data, poff.ctypes.data, cnt, loff.ctypes.data, docs.ctypes.data, tf.ctypes.data, total + 1,
                                         ctypes.byref(tot)) == 0

        def topk():
            assert L.sa_amd_index_doc_topk(ix._h, data.ctypes.data, poff.ctypes.data, cnt, args.k, loff.ctypes.data, tdocs.ctypes.data,
                                           ttf.ctypes.data) == 0
        say(f"\n{name}: occ_sum {int(occ.sum())}, df_sum {total}")
        l_ms = timed(listing, args.reps)
        f_ms = timed(freq, args.reps)
        st_f = sa.last_doc_tf_stats()
        assert st_f["tf_sum"] == int(occ.sum()) - sum(1 for p in pats if not p)
        k_ms = timed(topk, args.reps)
        st_k = sa.last_doc_tf_stats()
        lm, fm, km = statistics.median(l_ms), statistics.median(f_ms), statistics.median(k_ms)
        say(f"   doc_list {spread(l_ms)}   doc_tf {spread(f_ms)}   doc_topk {spread(k_ms)}   doc_tf / doc_list {fm / lm:.2f}   doc_topk / doc_list {km / lm:.2f}")
        lk, fk, kk = kernel_ms(listing), kernel_ms(freq), kernel_ms(topk)
        say(f"   kernels (ms, launches): doc_list {lk[0]:.3f}, {lk[1]}; doc_tf {fk[0]:.3f}, {fk[1]}; doc_topk {kk[0]:.3f}, {kk[1]}; "
            f"loads of S per listed document {st_f['table_loads'] / max(total, 1):.1f}; top-k: piece {st_k['piece']}, rounds {st_k['rounds']}, "
            f"pieces {st_k['pieces']}, entries {st_k['topk_entries']}")
        row = []
        for p in pieces:
            sa.docs_set_topk_piece(p)
            row.append(f"P = {p}: {spread(timed(topk, args.reps))} (kernels {kernel_ms(topk)[0]:.3f}, rounds {sa.last_doc_tf_stats()['rounds']})")
        sa.docs_set_topk_piece(-1)
        say("   doc_topk by piece: " + "; ".join(row))
        if can_ab:
            row = []
            for mode, label in ((0, "galloping"), (1, "plain")):
                L.sa_amd_debug_doc_tf_bounds(mode)
                ms = timed(freq, args.reps)
                row.append(f"{label}: {spread(ms)} (kernels {kernel_ms(freq)[0]:.3f}, loads of S per listed document "
                           f"{sa.last_doc_tf_stats()['table_loads'] / max(total, 1):.1f})")
            L.sa_amd_debug_doc_tf_bounds(0)
            say("   doc_tf by second bound: " + "; ".join(row))
    ix.close()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
