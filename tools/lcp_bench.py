"""LCP array timing: sa_amd_lcp_device on device-resident text + suffix array, per workload, beside the
suffix-array build of the same text, the LCP counters, the host-pointer routes and the CPU Kasai stand-in.

python tools/lcp_bench.py [--out DIR] [--calls K] [--only NAME,...] [--kasai-max-mib M]
Writes DIR/r05_lcp_table.txt and DIR/r05_lcp_table.csv (default DIR: profiles/).  Every result is checked: against Kasai where
it runs, otherwise against the closed form or 2 000 sampled slots compared on the host."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import Oracle


def fib(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return np.frombuffer(b[:n], dtype=np.uint8).copy()


M256 = 256 << 20
WORKLOADS = {
    "c2_uniform_256m": lambda: corpus.workload("c2_uniform_256m"),
    "c3_english_256m": lambda: corpus.workload("c3_english_256m"),
    "c4_dna_1g": lambda: corpus.workload("c4_dna_1g"),
    "all_one_byte_256m": lambda: np.full(M256, 97, dtype=np.uint8),
    "period2_256m": lambda: np.resize(np.frombuffer(b"ab", dtype=np.uint8), M256).copy(),
    "fibonacci_256m": lambda: fib(M256),
    "text_twice_256m": lambda: np.concatenate([corpus.english(M256 // 2, 5)] * 2),
    "dna_repeats_256m": lambda: corpus.dna_repeats(M256, 9, 0.4),
}


def kasai(orc, t, arr):
    L = orc.L
    L.oracle_lcp_kasai.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.oracle_lcp_kasai.restype = ctypes.c_int32
    out = np.zeros(t.size + 1, dtype=np.uint32)
    t0 = time.perf_counter()
    assert L.oracle_lcp_kasai(t.ctypes.data, t.size, arr.ctypes.data, out.ctypes.data) == 0
    return out, (time.perf_counter() - t0) * 1e3


def sampled_ok(t, arr, got, samples=2000):
    rng = np.random.default_rng(1)
    for i in rng.integers(1, t.size + 1, samples):
        a, b, h = int(arr[i - 1]), int(arr[i]), int(got[i])
        x, y = t[a:a + h + 1], t[b:b + h + 1]
        if not np.array_equal(x[:h], y[:h]) or not (x.size == h or y.size == h or x[h] != y[h]):
            return False
    return True


def med_spread(xs):
    return statistics.median(xs), max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--kasai-max-mib", type=int, default=256)
    ap.add_argument("--no-host", action="store_true", help="skip the host-pointer routes")
    args = ap.parse_args()
    names = [k for k in WORKLOADS if not args.only or k in args.only.split(",")]
    orc = Oracle()
    rows = []
    hdr = ("workload", "n", "lcp_ms", "lcp_spread_ms", "lcp_GBps", "sa_build_ms", "lcp_over_sa", "irreducible", "compared_bytes",
           "long_pairs", "readbacks", "host_lcp_ms", "host_saca_lcp_ms", "cpu_kasai_ms", "check")
    for name in names:
        t = np.ascontiguousarray(WORKLOADS[name]())
        n = t.size
        dT = torch.from_numpy(t).to("cuda")
        dS = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        dL = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        wsa = sa.workspace_bytes(n)
        wl = sa.lcp_work_bytes(n)
        dW = torch.empty(max(wsa, wl), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sa_ms = []
        for k in range(args.calls + 1):
            t0 = time.perf_counter()
            sa.saca_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dW.data_ptr(), wsa)
            torch.cuda.synchronize()
            if k:
                sa_ms.append((time.perf_counter() - t0) * 1e3)
        lcp_ms = []
        for k in range(args.calls + 1):
            t0 = time.perf_counter()
            sa.lcp_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dL.data_ptr(), dW.data_ptr(), wl)
            torch.cuda.synchronize()
            if k:
                lcp_ms.append((time.perf_counter() - t0) * 1e3)
        st = sa.last_lcp_stats()
        arr = dS.cpu().numpy().view(np.uint32)
        got = dL.cpu().numpy().view(np.uint32)
        del dT, dS, dL, dW
        torch.cuda.empty_cache()
        host_ms = sc_ms = float("nan")
        if not args.no_host:
            hs, ss = [], []
            for _ in range(2):
                t0 = time.perf_counter(); h1 = sa.lcp(t, arr); hs.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); a2, h2 = sa.saca_lcp(t); ss.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(h1, got) and np.array_equal(h2, got) and np.array_equal(a2, arr), name
            host_ms, sc_ms = min(hs), min(ss)
            del h1, h2, a2
            sa.lib().sa_amd_release_cache()
        if n <= (args.kasai_max_mib << 20):
            exp, k_ms = kasai(orc, t, arr)
            check = "kasai" if np.array_equal(exp, got) else "MISMATCH"
            del exp
        else:
            k_ms = float("nan")
            check = "sampled" if sampled_ok(t, arr, got) else "MISMATCH"
        m, sp = med_spread(lcp_ms)
        sm, _ = med_spread(sa_ms)
        row = (name, n, round(m, 2), round(sp, 2), round(n / (m * 1e6), 1), round(sm, 2), round(m / sm, 2), st["irreducible"],
               st["compared_bytes"], st["long_pairs"], st["readbacks"], round(host_ms, 1), round(sc_ms, 1), round(k_ms, 0), check)
        rows.append(row)
        print("  ".join(f"{h}={v}" for h, v in zip(hdr, row)), flush=True)
        del arr, got, t
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "r05_lcp_table.csv"), "w") as f:
        f.write(",".join(hdr) + "\n")
        for r in rows:
            f.write(",".join(str(v) for v in r) + "\n")
    with open(os.path.join(args.out, "r05_lcp_table.txt"), "w") as f:
        f.write(f"tools/lcp_bench.py  ({torch.cuda.get_device_name(0)}; median and spread of {args.calls} calls after one warm-up, "
                "each ending in a device synchronise; lcp_GBps = input bytes / lcp time; host_* = best of 2 end-to-end host-pointer "
                "calls; cpu_kasai_ms = oracle_lcp_kasai on one core, the stand-in for the CPU route)\n")
        f.write(f"{'workload':20s} {'n':>11s} {'lcp ms':>8s} {'+-':>6s} {'GB/s':>6s} {'SA ms':>8s} {'LCP/SA':>6s} {'irreducible':>11s} "
                f"{'compared B':>12s} {'long':>6s} {'rb':>3s} {'sa_amd_lcp':>10s} {'saca_u8_lcp':>11s} {'Kasai ms':>9s} check\n")
        for r in rows:
            f.write(f"{r[0]:20s} {r[1]:>11d} {r[2]:>8.2f} {r[3]:>6.2f} {r[4]:>6.1f} {r[5]:>8.2f} {r[6]:>6.2f} {r[7]:>11d} {r[8]:>12d} "
                    f"{r[9]:>6d} {r[10]:>3d} {r[11]:>10.1f} {r[12]:>11.1f} {r[13]:>9.0f} {r[14]}\n")
    return 0 if all(r[-1] != "MISMATCH" for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
