"""DESIGN.md section 15, measured: matching statistics and shared spans of a query against the device index (kernels/match.hpp)
against the only route there was before -- sa_amd_index_search on the explicit windows of the same query, one wave a window.

python tools/match_bench.py [--workloads c3_english_256m,dna_256m] [--query-mib 16] [--caps 16,32,64,256] [--reps 5]
                            [--groups 4,8,16] [--out profiles/match_stats.txt]

Per workload two queries: a held-out slice of the same generator (another seed) and a slice of the text with 1 % of its bytes
substituted.  Per cap C: match_stats host to host, match_stats device-resident, match_spans at k = 50 (host to host), each the
median of --reps calls after a warm-up with min..max; the baseline in chunks of 2^20 windows, one run, the calls alone timed
(the windows are cut on the host beforehand): with the window upload, and less the time a copy of that many bytes takes,
measured apart.  Every run's ML and POS are compared in full against the baseline's lcp_len / lcp_start wherever lcp_len > 0.  G, the
lanes of a group, is switched through match_set_group_lanes for the A/B at the end of each block."""
import argparse
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

M256 = 256 << 20
WORKLOADS = {
    "c3_english_256m": (lambda n: corpus.english_corpus(n, 3), lambda m: corpus.english_corpus(m, 1003)),
    "dna_256m": (lambda n: corpus.dna(n, 4), lambda m: corpus.dna(m, 1004)),
}
CHUNK = 1 << 20


def spread(xs):
    return f"{statistics.median(xs):9.2f} ({min(xs):.2f}..{max(xs):.2f})"


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


def windows(q, j0, j1, cap):
    m = q.size
    lens = np.minimum(cap, m - np.arange(j0, j1))
    off = np.zeros(j1 - j0 + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    if j1 + cap <= m + 1:
        data = np.lib.stride_tricks.sliding_window_view(q, cap)[j0:j1].reshape(-1).copy()
    else:
        data = np.concatenate([q[j:j + cap] for j in range(j0, j1)])
    return data, off


def baseline(ix, q, cap):
    """-> (lcp_len, lcp_start, ms with the window upload, ms of building nothing but the call: windows prepared beforehand)"""
    m = q.size
    ll, ls = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    call_ms = 0.0
    L = sa.lib()
    for j0 in range(0, m, CHUNK):
        j1 = min(m, j0 + CHUNK)
        data, off = windows(q, j0, j1, cap)
        t0 = time.perf_counter()
        rc = L.sa_amd_index_search(ix._h, data.ctypes.data, off.ctypes.data, j1 - j0, None, None, None, ls[j0:].ctypes.data, ll[j0:].ctypes.data)
        call_ms += (time.perf_counter() - t0) * 1e3
        assert rc == 0
    return ll, ls, call_ms


def upload_ms(nbytes):
    host = torch.empty(min(nbytes, 1 << 28), dtype=torch.uint8)
    dev = torch.empty_like(host, device="cuda")
    dev.copy_(host)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev.copy_(host)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 * nbytes / host.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--index-mib", type=int, default=256)
    ap.add_argument("--query-mib", type=float, default=16)
    ap.add_argument("--caps", default="16,32,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="4,8,16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    n, m = args.index_mib << 20, int(args.query_mib * (1 << 20))
    caps = [int(c) for c in args.caps.split(",")]
    say(f"device: {sa.device_pci_bus_id(0)}; index {args.index_mib} MiB, query {m} bytes; ms, median of {args.reps} calls after a warm-up "
        f"(min..max); baseline = sa_amd_index_search on the explicit windows, {CHUNK} a call, one run")
    for name in args.workloads.split(","):
        make_t, make_q = WORKLOADS[name]
        t = make_t(n)
        rng = np.random.default_rng(7)
        start = int(rng.integers(0, n - m))
        near = t[start:start + m].copy()
        hit = rng.random(m) < 0.01
        near[hit] ^= np.uint8(1)
        ix = sa.DeviceIndex(t)
        for qname, q in (("held-out", make_q(m)), ("1% substituted", near)):
            say(f"\n== {name}, query {qname}")
            say(f"{'C':>5} {'G':>3} {'stats host ms':>26} {'stats device ms':>26} {'spans k=50 ms':>26} {'baseline ms':>12} {'- upload':>9} "
                f"{'speed-up':>8} {'cmp B/pos':>9} {'steps/pos':>9} {'long':>9} {'mean ML':>8}")
            dQ = torch.from_numpy(q).cuda()
            dM = torch.empty(m, dtype=torch.int32, device="cuda")
            dP = torch.empty(m, dtype=torch.int32, device="cuda")
            wb = sa.match_work_bytes(m)
            dW = torch.empty(wb, dtype=torch.uint8, device="cuda")
            for cap in caps:
                ll, ls, base_ms = baseline(ix, q, cap)
                up = upload_ms(int(np.minimum(cap, m - np.arange(m)).sum()))
                on = ll > 0
                for G in [int(g) for g in args.groups.split(",")]:
                    sa.match_set_group_lanes(G)
                    res = {}
                    host = timed(lambda: res.__setitem__("h", ix.match_stats(q, cap)), args.reps)
                    st = sa.last_match_stats()
                    dev = timed(lambda: sa.match_stats_device_ptr(ix, dQ.data_ptr(), m, cap, dM.data_ptr(), dP.data_ptr(), dW.data_ptr(), wb), args.reps)
                    spans = timed(lambda: res.__setitem__("s", ix.match_spans(q, 50)), args.reps)
                    assert st["group_lanes"] == G
                    for ml, pos in (res["h"], (dM.cpu().numpy().view(np.uint32), dP.cpu().numpy().view(np.uint32))):
                        assert np.array_equal(ml > 0, on) and np.array_equal(ml[on], ll[on]) and np.array_equal(pos[on], ls[on]), (name, qname, cap, G)
                    say(f"{cap:5d} {G:3d} {spread(host):>26} {spread(dev):>26} {spread(spans):>26} {base_ms:12.1f} {base_ms - up:9.1f} "
                        f"{(base_ms - up) / statistics.median(dev):8.2f} {st['compared_bytes'] / m:9.1f} {st['steps'] / m:9.2f} "
                        f"{st['long_positions']:9d} {st['ml_sum'] / m:8.2f}")
                sa.match_set_group_lanes(-1)
        ix.close()
        del t
        sa.lib().sa_amd_release_cache()
    if args.out:
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
