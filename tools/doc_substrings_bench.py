"""DESIGN.md section 20, measured: repeated substrings with their document frequency (sa_amd_index_doc_substrings) beside
sa_amd_index_substrings with the same first five fields of the query, on the same index, in the same run.

python tools/doc_substrings_bench.py [--mib 256] [--doc-bytes 4096] [--huge 8] [--calls 3] [--only NAME,...]
                                     [--lib libsuffix_array_amd_diag.so] [--out DIR]
Writes DIR/doc_substrings_table.txt (default DIR: profiles/).  Workloads: the English-like corpus and DNA, cut into documents
of about --doc-bytes bytes (random lengths), and the English-like corpus once more as --huge documents.  Times are the median
of --calls calls after a warm-up, each ending in a device synchronise, results copied to the host as a caller sees them.
table_ms is HIP-event time: the class k_rep_spans of the call less that class of the plain call -- the pair pass, the scan and
the node pass's two more loads.  200 sampled rows of every timed query are checked against doc_search.  The A/B of the pair pass
(equal targets combined inside a wave against one atomic per pair) needs the diagnostic library's switch: it runs when --lib
names that library."""
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

QUERIES = (("cover_k65536_max16_docs2", dict(min_len=1, max_len=16, min_count=2, order=sa.SUBSTR_BY_COVER, k=65536), 2),
           ("length_k1000_min50_docs2", dict(min_len=50, max_len=0, min_count=2, order=sa.SUBSTR_BY_LENGTH, k=1000), 2))


def class_ms(fn):
    """device time per profile class of one call (HIP events on the launch stream)"""
    L = sa.lib()
    names = []
    while L.sa_amd_profile_kernel_name(len(names)):
        names.append(L.sa_amd_profile_kernel_name(len(names)).decode())
    L.sa_amd_profile_begin()
    fn()
    ms, launches, units = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)(), (ctypes.c_int64 * 64)()
    cnt = L.sa_amd_profile_end(ms, launches, units, 64)
    return {names[i]: ms[i] for i in range(min(cnt, len(names)))}


def timed(fn, calls):
    xs = []
    for k in range(calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            xs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(xs), max(xs) - min(xs)


def cut(n, docs, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate(([0], np.sort(rng.integers(0, n + 1, docs - 1)), [n])).astype(np.int64)


def sampled_ok(ix, t, rows, df, pos, samples=200):
    if rows.shape[0] == 0:
        return True
    pick = np.random.default_rng(1).integers(0, rows.shape[0], samples)
    occ, want = ix.doc_search([t[int(pos[r]):int(pos[r]) + int(rows[r, 2])].tobytes() for r in pick])
    return bool(np.array_equal(occ, rows[pick, 1]) and np.array_equal(want, df[pick]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--doc-bytes", type=int, default=4096)
    ap.add_argument("--huge", type=int, default=8)
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.lib:
        sa._LIB_NAME = args.lib                                       # (before the first call: the library is loaded once)
    L = sa.lib()
    can_ab = hasattr(ctypes.CDLL(sa.library_path()), "sa_amd_debug_dsub_plain_atomics")
    n = args.mib << 20
    small = max(n // args.doc_bytes, 1)
    english, dna = (lambda: corpus.workload("c3_english_256m", n_override=n)), (lambda: corpus.dna(n, 4))
    works = (("english_%dm" % args.mib, english, small), ("english_%dm_huge" % args.mib, english, args.huge), ("dna_%dm" % args.mib, dna, small))
    hdr = ("workload", "ndocs", "query", "n", "doc_substrings_ms", "spread_ms", "substrings_ms", "ratio", "table_ms", "rep_spans_ms",
           "plain_atomics_ms", "plain_atomics_table_ms", "total", "selected", "df_sum", "max_df", "pairs", "rmq_far_share", "steps_per_pair",
           "rmq_max", "readbacks", "check")
    lines = []
    t = made = None
    for name, make, ndocs in works:
        if args.only and name not in args.only.split(","):
            continue
        if made is not make:
            t, made = np.ascontiguousarray(make()), make
        ix = sa.DeviceIndex(t)
        ix.set_documents(cut(n, ndocs, 5))
        for qname, q, md in QUERIES:
            got = []

            def doc_call():
                got[:] = ix.doc_substrings(min_docs=md, positions=True, **q)

            def plain_call():
                ix.repeated_substrings(**q)
            pm, _ = timed(plain_call, args.calls)
            plain_cls = class_ms(plain_call)
            dm, dsp = timed(doc_call, args.calls)
            st = sa.last_doc_substr_stats()
            cls = class_ms(doc_call)
            table = cls.get("k_rep_spans", 0.0) - plain_cls.get("k_rep_spans", 0.0)
            am = at = "n/a"
            if can_ab:
                L.sa_amd_debug_dsub_plain_atomics(1)
                am = round(timed(doc_call, args.calls)[0], 2)
                at = round(class_ms(doc_call).get("k_rep_spans", 0.0) - plain_cls.get("k_rep_spans", 0.0), 2)
                L.sa_amd_debug_dsub_plain_atomics(0)
                doc_call()
            rows, df, pos = got
            row = (name, ndocs, qname, n, round(dm, 2), round(dsp, 2), round(pm, 2), round(dm / pm, 2), round(table, 2),
                   round(cls.get("k_rep_spans", 0.0), 2), am, at, rows.shape[0], st["selected"], st["df_sum"], st["max_df"], st["pairs"],
                   round(st["rmq_far"] / max(st["pairs"], 1), 4), round(st["rmq_steps"] / max(st["pairs"], 1), 1), st["rmq_max"], st["readbacks"],
                   "sampled" if sampled_ok(ix, t, rows, df, pos) else "MISMATCH")
            lines.append("  ".join(f"{h}={v}" for h, v in zip(hdr, row)))
            print(lines[-1], flush=True)
        ix.close()
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "doc_substrings_table.txt"), "w") as f:
        f.write(f"tools/doc_substrings_bench.py  ({torch.cuda.get_device_name(0)}, library {os.path.basename(sa.library_path())}; median and spread of "
                f"{args.calls} calls after one warm-up, each ending in a device synchronise, results copied to the host; substrings_ms = "
                "sa_amd_index_substrings with the same first five fields on the same index in the same run; rep_spans_ms = HIP-event time of the "
                "class k_rep_spans of one more call, table_ms = that less the plain call's: the pair pass, the scan and the node pass's two more "
                "loads; plain_atomics_* = the same with one atomic per pair instead of one per distinct target of a wave)\n")
        for ln in lines:
            f.write(ln + "\n")
    return 0 if all("MISMATCH" not in ln for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
