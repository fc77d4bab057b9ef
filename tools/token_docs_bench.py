"""DESIGN.md section 27, measured: document collections over the token indexes, beside what a user of a token index did before
-- search, download of the ranges' slice of the suffix array, np.searchsorted into the offsets, np.unique on the host -- and, for
the separator pass, beside np.flatnonzero on the host with the upload of the offsets.

python tools/token_docs_bench.py [--tokens 16777216] [--doc-tokens 512] [--patterns 1000] [--reps 5] [--out profiles/token_docs_table.txt]

The texts are corpus.token_corpus (16-bit) and corpus.token_corpus_u32 (32-bit) with an id the text does not hold written at
seeded random positions, one every --doc-tokens tokens on average: the separator.  Patterns are n-grams of 1 .. 4 tokens read
from the text.  Every library call blocks until its answer is on the host, so a time is the wall clock of the call; the median of
--reps calls after a warm-up, with min..max.  No figure is a threshold of anything."""
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
from suffix_array_amd import Not, corpus


def spread(xs):
    return f"{statistics.median(xs):10.3f} ({min(xs):.3f}..{max(xs):.3f})"


def timed(fn, reps):
    fn()                                                              # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def text_of(width, n, doc_tokens, seed):
    t = corpus.token_corpus(n, 50000, seed) if width == 16 else corpus.token_corpus_u32(n, 128000, seed)
    absent = np.setdiff1d(np.arange(1 << 16, dtype=np.int64), np.unique(t), assume_unique=True)
    sep = int(absent[-1])
    rng = np.random.default_rng(seed + 1)
    t = t.copy()
    t[rng.integers(0, n, max(n // doc_tokens, 1))] = sep
    return t, sep


def run(width, args, lines):
    cls = sa.TokenIndex if width == 16 else sa.TokenIndex32
    n = args.tokens
    t, sep = text_of(width, n, args.doc_tokens, 5)
    t0 = time.perf_counter()
    ix = cls(t)
    build_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(9)
    pats = []
    for _ in range(args.patterns):
        k, a = int(rng.integers(1, 5)), int(rng.integers(0, n - 4))
        pats.append(t[a:a + k].copy())
    queries = [[pats[i], pats[i + 1]] if i % 2 else [pats[i], Not(pats[i + 1])] for i in range(0, args.patterns - 1, 2)]
    P, Q = len(pats), len(queries)

    def host_offsets():
        off = np.concatenate(([0], np.flatnonzero(t == sep) + 1, [n] if t[-1] != sep else [])).astype(np.uint32)
        ix.set_documents(off)
        return off
    flat_ms = timed(lambda: np.flatnonzero(t == sep), args.reps)
    host_ms = timed(host_offsets, args.reps)
    off = host_offsets()
    by_off = timed(lambda: ix.set_documents(off), args.reps)
    by_sep = timed(lambda: ix.set_documents(separator=sep), args.reps)
    assert np.array_equal(ix.doc_offsets(), off)
    ndocs = ix.ndocs
    search_ms = timed(lambda: ix.doc_search(pats), args.reps)
    list_ms = timed(lambda: ix.doc_list(pats), args.reps)
    match_ms = timed(lambda: ix.doc_match(queries), args.reps)
    mlist_ms = timed(lambda: ix.doc_match_list(queries), args.reps)
    arr_ms = timed(lambda: ix.sa(), 1)
    arr = ix.sa()
    lo, hi = ix.search(pats)
    off64 = off.astype(np.int64)

    def host_df():
        lo2, hi2 = ix.search(pats)
        return [np.unique(np.searchsorted(off64, arr[a:b].astype(np.int64), "right") - 1) for a, b in zip(lo2.tolist(), hi2.tolist())]
    host_df_ms = timed(host_df, args.reps)
    occ, df = ix.doc_search(pats)
    want = host_df()
    assert [w[w < ndocs].size for w in want] == df.tolist() and np.array_equal(occ, hi - lo)
    assert all(np.array_equal(np.sort(g), w[w < ndocs]) for g, w in zip(ix.doc_list(pats), want))
    ds = sa.last_docs_stats()
    lines.append(f"{width}-bit tokens: n = {n} tokens, separator {sep}, ndocs = {ndocs}; index build {build_ms:.1f} ms; {P} patterns of 1..4 tokens "
                 f"(occ_sum {int(occ.sum())}, df_sum {int(df.sum())}, {ds['units']} units of the listing call), {Q} two-clause queries")
    lines.append(f"  set_documents(offsets)            {spread(by_off)} ms   ({(ndocs + 1) * 4 / 2**20:.1f} MiB of offsets up)")
    lines.append(f"  set_documents(separator=)         {spread(by_sep)} ms   (the text read twice on the device: {2 * t.itemsize * n / 2**20:.0f} MiB)")
    lines.append(f"    host: np.flatnonzero alone      {spread(flat_ms)} ms;  flatnonzero + concatenate + set_documents(offsets) {spread(host_ms)} ms")
    lines.append(f"  doc_search                        {spread(search_ms)} ms   = {statistics.median(search_ms) * 1e3 / P:8.2f} us a pattern")
    lines.append(f"  doc_list                          {spread(list_ms)} ms   = {statistics.median(list_ms) * 1e3 / P:8.2f} us a pattern")
    lines.append(f"  doc_match                         {spread(match_ms)} ms   = {statistics.median(match_ms) * 1e3 / Q:8.2f} us a query")
    lines.append(f"  doc_match_list                    {spread(mlist_ms)} ms   = {statistics.median(mlist_ms) * 1e3 / Q:8.2f} us a query")
    lines.append(f"  before: search + searchsorted + unique on the host, the array already down {spread(host_df_ms)} ms "
                 f"= {statistics.median(host_df_ms) * 1e3 / P:8.2f} us a pattern; the array's download, once: {arr_ms[0]:.1f} ms; answers equal")
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 24)
    ap.add_argument("--doc-tokens", type=int, default=512)
    ap.add_argument("--patterns", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_docs_table.txt"))
    args = ap.parse_args()
    name = (ctypes.c_char * 256)()
    device = "device 0"
    if sa.lib().sa_amd_device_pci_bus_id(0, name, 256) == 0:
        device = "device " + name.value.decode()
    lines = [f"tools/token_docs_bench.py: {device}, library {os.path.basename(sa.library_path())}; --tokens {args.tokens} --doc-tokens {args.doc_tokens} "
             f"--patterns {args.patterns}; ms, median of {args.reps} calls after a warm-up (min..max)", ""]
    for width in (16, 32):
        run(width, args, lines)
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
