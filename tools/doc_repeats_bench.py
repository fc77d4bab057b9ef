"""DESIGN.md section 17, measured: document-aware duplicate spans over the device index (kernels/doc_repeats.hpp) against the
boundary-blind sa_amd_index_repeat_spans(KEEP_FIRST) of the same index in the same process -- the capability there was before,
which shares the LCP front end.

python tools/doc_repeats_bench.py [--index-mib 256] [--docs 65536] [--min-len 50] [--reps 5] [--out profiles/doc_repeats_bench.txt]

The text is the English-like corpus of bench.py (corpus.english_corpus(n, 3)), cut into --docs equal documents.  Times are the
median of --reps calls after a warm-up, each ending in a device synchronise, with min..max; kernel times are the summed HIP
event times of the library's own profile (sa_amd_profile_begin / _end) in one more call: the classes k_rep_lr (slot pass, spine,
mark), k_rep_spans (the five span passes and the accounting pass) and misc (the count of touched documents) are this feature's
(and the yardstick's own slot / mark / span passes), every other class is the LCP front end."""
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

MODES = {sa.REPEATS_ALL: "ALL", sa.REPEATS_KEEP_FIRST: "KEEP_FIRST"}
SCOPES = {sa.DOCREP_ANY: "ANY", sa.DOCREP_OTHER: "OTHER"}
OWN = ("k_rep_lr", "k_rep_spans", "misc")


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
    ap.add_argument("--min-len", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n = args.index_mib << 20
    k = args.min_len
    t = corpus.english_corpus(n, 3)
    off = (np.arange(args.docs + 1, dtype=np.int64) * n) // args.docs
    say(f"tools/doc_repeats_bench.py: {torch.cuda.get_device_name(0)}; English-like text of {args.index_mib} MiB in {args.docs} equal documents, "
        f"min_len {k}; ms, median of {args.reps} calls after a warm-up (min..max)")
    ix = sa.DeviceIndex(t)
    ix.set_documents(off)
    L = sa.lib()
    cap = sa.repeat_spans_bound(n, k)
    spans = np.empty((cap, 2), dtype=np.uint32)
    db = np.zeros(args.docs, dtype=np.uint32)
    count = ctypes.c_int64(0)
    say(f"scratch from the pool: {sa.doc_repeats_work_bytes(n, args.docs) / 2**30:.2f} GiB (sa_amd_index_repeat_spans: {sa.repeats_work_bytes(n) / 2**30:.2f} GiB)")

    def blind():
        assert L.sa_amd_index_repeat_spans(ix._h, k, sa.REPEATS_KEEP_FIRST, spans.ctypes.data, cap, ctypes.byref(count)) == 0

    def split_of(fn):
        sp = kernel_split(fn)
        own = sum(v[0] for name, v in sp.items() if name in OWN)
        front = sum(v[0] for name, v in sp.items() if name not in OWN)
        return sp, own, front

    y = timed(blind, args.reps)
    ysp, yown, yfront = split_of(blind)
    ys = sa.last_repeat_stats()
    say(f"\nyardstick sa_amd_index_repeat_spans(KEEP_FIRST, {k}): {spread(y)} ms; kernels: front end {yfront:.3f} ms, its own passes {yown:.3f} ms")
    say(f"   spans {ys['spans']}, flagged {ys['flagged']}, covered {ys['covered_bytes']}; classes (ms, launches): {ysp}")
    say(f"\n{'mode':>10} {'scope':>6} {'doc_bytes':>9} {'call ms':>28} {'less yardstick':>14} {'front end ms':>12} {'rep_lr ms':>10} {'rep_spans ms':>12} {'misc ms':>8}"
        f" {'members':>10} {'flagged':>10} {'spans':>8} {'covered':>10} {'touched':>8}")
    for mode in MODES:
        for scope in SCOPES:
            for with_db in (False, True):
                def call():
                    assert L.sa_amd_index_doc_repeat_spans(ix._h, k, mode, scope, spans.ctypes.data, cap, ctypes.byref(count),
                                                           db.ctypes.data if with_db else None) == 0
                c = timed(call, args.reps)
                sp, own, front = split_of(call)
                st = sa.last_doc_repeat_stats()
                if with_db:
                    assert int(db.sum(dtype=np.int64)) == st["covered_bytes"] and int(np.count_nonzero(db)) == st["docs_touched"]
                g = lambda name: sp.get(name, (0.0, 0))[0]
                say(f"{MODES[mode]:>10} {SCOPES[scope]:>6} {'yes' if with_db else 'no':>9} {spread(c):>28} {statistics.median(c) - statistics.median(y):14.3f} "
                    f"{front:12.3f} {g('k_rep_lr'):10.3f} {g('k_rep_spans'):12.3f} {g('misc'):8.3f} {st['members']:10d} {st['flagged']:10d} {st['spans']:8d} "
                    f"{st['covered_bytes']:10d} {st['docs_touched']:8d}")
    sp, own, front = split_of(lambda: ix.doc_repeat_spans(k, doc_bytes=True))
    say(f"\nclasses of one KEEP_FIRST / OTHER call with doc_bytes (ms, launches): {sp}")
    one = [0, n]
    ix.set_documents(one)                                             # the ndocs = 1 identity at this size
    a = ix.doc_repeat_spans(k, sa.REPEATS_KEEP_FIRST, sa.DOCREP_ANY)
    b = ix.repeat_spans(k, keep_first=True)
    assert np.array_equal(a, b)
    say(f"one document, scope ANY: the {a.shape[0]} spans of sa_amd_index_repeat_spans(KEEP_FIRST), bit for bit")
    ix.close()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
