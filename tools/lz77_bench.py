"""LZ77 factorisation timing: sa_amd_lz77_device and sa_amd_lpf_device on device-resident text + suffix
array, per workload, with the time of every stage, beside sa_amd_lcp_device and the suffix-array build of the same text, the
stage-1 and walk counters, compared_bytes / (n log2 n), and a single-core CPU baseline (oracle_lz77 of oracle/oracle.c).

python tools/lz77_bench.py [--out DIR] [--calls K] [--only NAME,...] [--cpu-max-mib M]
Writes DIR/r09_lz77_table.txt and DIR/r09_lz77_table.csv (default DIR: profiles/).  Every parse is checked: against the CPU
baseline where it runs, otherwise by decoding 200 sampled phrases against the text."""
import argparse
import ctypes
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import suffix_array_amd as sa
from suffix_array_amd import corpus

M256 = 256 << 20
STAGES = (("nsv", ("k_lcp_phi",)), ("values", ("k_lcp_irreducible", "k_lcp_long", "k_lcp_scan")), ("walk", ("k_unbwt_walk", "k_unbwt_rank", "k_unbwt_write")),
          ("merge_emit", ("k_rep_spans",)))


def fib(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return np.frombuffer(b[:n], dtype=np.uint8).copy()


WORKLOADS = {
    "c3_english_256m": lambda: corpus.workload("c3_english_256m"),
    "c2_uniform_256m": lambda: corpus.workload("c2_uniform_256m"),
    "c4_dna_1g": lambda: corpus.workload("c4_dna_1g"),
    "all_one_byte_256m": lambda: np.full(M256, 97, dtype=np.uint8),
    "period2_256m": lambda: np.resize(np.frombuffer(b"ab", dtype=np.uint8), M256).copy(),
    "fibonacci_256m": lambda: fib(M256),
    "text_twice_256m": lambda: np.concatenate([corpus.english(M256 // 2, 5)] * 2),
}


def cpu_lib():
    """the oracle library's linear-time factorisation: the same code the test suite checks the device against"""
    so = os.path.join(ROOT, "oracle", "liboracle.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "all"], cwd=os.path.join(ROOT, "oracle"))
    L = ctypes.CDLL(so)
    L.oracle_lz77.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_int64]
    L.oracle_lz77.restype = ctypes.c_int64
    return L


def stage_ms(fn):
    """per-stage device time of one call from the profile classes the factorisation's kernels are charged to"""
    L = sa.lib()
    names = []
    while L.sa_amd_profile_kernel_name(len(names)):
        names.append(L.sa_amd_profile_kernel_name(len(names)).decode())
    L.sa_amd_profile_begin()
    fn()
    ms, launches, units = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)(), (ctypes.c_int64 * 64)()
    cnt = L.sa_amd_profile_end(ms, launches, units, 64)
    got = {names[i]: ms[i] for i in range(min(cnt, len(names)))}
    return {stage: sum(got.get(k, 0.0) for k in ks) for stage, ks in STAGES}


def timed(fn, calls):
    xs = []
    for k in range(calls + 1):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            xs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(xs), max(xs) - min(xs)


def sampled_ok(t, ph, samples=200):
    starts = np.cumsum(ph[:, 1].astype(np.int64)) - ph[:, 1]
    rng = np.random.default_rng(1)
    for k in rng.integers(0, ph.shape[0], samples):
        s, (q, ln) = int(starts[k]), (int(ph[k, 0]), int(ph[k, 1]))
        if q == sa.LZ_LITERAL:
            if ln != 1:
                return False
            continue
        m = min(ln, 4096)
        if not (q < s and np.array_equal(t[q:q + m], t[s:s + m]) and np.array_equal(t[q + ln - m:q + ln], t[s + ln - m:s + ln])):
            return False
        if s + ln < t.size and t[q + ln] == t[s + ln]:                # greedy: the match does not go on
            return False
    return int(starts[-1] + ph[-1, 1]) == t.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--cpu-max-mib", type=int, default=256)
    args = ap.parse_args()
    names = [k for k in WORKLOADS if not args.only or k in args.only.split(",")]
    cpu = cpu_lib()
    hdr = ("workload", "n", "lz77_ms", "spread_ms", "lpf_ms", "lcp_ms", "lz77_over_lcp", "sa_build_ms", "nsv_ms", "values_ms", "walk_ms",
           "merge_emit_ms", "phrases", "literals", "longest", "unresolved_share", "steps_per_unresolved", "hierarchy_max", "walkers",
           "walk_launches", "restarts", "irreducible", "compared_bytes", "bytes_per_nlog2n", "readbacks", "cpu_ms", "check")
    rows = []
    for name in names:
        t = np.ascontiguousarray(WORKLOADS[name]())
        n = t.size
        dT = torch.from_numpy(t).to("cuda")
        dS = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        wsa, wl, wz = sa.workspace_bytes(n), sa.lcp_work_bytes(n), sa.lz_work_bytes(n)
        dW = torch.empty(max(wsa, wl, wz), dtype=torch.uint8, device="cuda")
        dL = torch.empty(2 * (n + 1), dtype=torch.int32, device="cuda")
        cap = n
        dP = torch.empty(2 * min(cap, 1 << 28), dtype=torch.int32, device="cuda")
        cap = dP.numel() // 2
        torch.cuda.synchronize()
        sm, _ = timed(lambda: sa.saca_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dW.data_ptr(), wsa), args.calls)
        lm, _ = timed(lambda: sa.lcp_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dL.data_ptr(), dW.data_ptr(), wl), args.calls)
        pm, _ = timed(lambda: sa.lpf_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dL.data_ptr(), dL.data_ptr() + 4 * (n + 1), dW.data_ptr(), wz),
                      args.calls)
        count = []
        zm, zsp = timed(lambda: count.append(sa.lz77_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dP.data_ptr(), cap, dW.data_ptr(), wz)), args.calls)
        st, ls = sa.last_lz_stats(), sa.last_lcp_stats()
        stages = stage_ms(lambda: sa.lz77_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dP.data_ptr(), cap, dW.data_ptr(), wz))
        z = count[-1]
        ph = dP[:2 * min(z, cap)].cpu().numpy().view(np.uint32).reshape(-1, 2)
        arr = dS.cpu().numpy().view(np.uint32)
        del dT, dS, dL, dP, dW
        torch.cuda.empty_cache()
        cpu_ms = float("nan")
        if n <= (args.cpu_max_mib << 20):
            lpf, src = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
            exp = np.empty((min(z, cap), 2), dtype=np.uint32)
            t0 = time.perf_counter()
            zc = cpu.oracle_lz77(t.ctypes.data, n, arr.ctypes.data, lpf.ctypes.data, src.ctypes.data, exp.ctypes.data, exp.shape[0])
            cpu_ms = (time.perf_counter() - t0) * 1e3
            check = "cpu" if zc == z and np.array_equal(exp, ph) else "MISMATCH"
            del lpf, src, exp
        else:
            check = "sampled" if z <= cap and sampled_ok(t, ph) else "MISMATCH"
        row = (name, n, round(zm, 2), round(zsp, 2), round(pm, 2), round(lm, 2), round(zm / lm, 2), round(sm, 2),
               round(stages["nsv"], 2), round(stages["values"], 2), round(stages["walk"], 2), round(stages["merge_emit"], 2),
               st["phrases"], st["literals"], st["longest"], round(st["unresolved"] / n, 4),
               round(st["hierarchy_steps"] / max(st["unresolved"], 1), 1), st["hierarchy_max"], st["walkers"], st["walk_launches"],
               st["restarts"], ls["irreducible"], ls["compared_bytes"], round(ls["compared_bytes"] / (n * math.log2(n)), 3),
               st["readbacks"], round(cpu_ms, 0), check)
        rows.append(row)
        print("  ".join(f"{h}={v}" for h, v in zip(hdr, row)), flush=True)
        del arr, ph, t
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "r09_lz77_table.csv"), "w") as f:
        f.write(",".join(hdr) + "\n")
        for r in rows:
            f.write(",".join(str(v) for v in r) + "\n")
    with open(os.path.join(args.out, "r09_lz77_table.txt"), "w") as f:
        f.write(f"tools/lz77_bench.py  ({torch.cuda.get_device_name(0)}; median and spread of {args.calls} calls after one warm-up, each ending "
                "in a device synchronise; array resident; *_ms stage columns: HIP-event time of one more call, the range pass counted with nsv; "
                "cpu_ms = oracle_lz77 (oracle/oracle.c) on one core, array given)\n")
        for r in rows:
            f.write("  ".join(f"{h}={v}" for h, v in zip(hdr, r)) + "\n")
    return 0 if all(r[-1] != "MISMATCH" for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
