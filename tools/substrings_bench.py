"""Repeated-substring enumeration timing: sa_amd_substrings_device on device-resident text + suffix array,
per workload and query, beside sa_amd_lcp_device and the suffix-array build of the same text in the same run, with the device
time of every stage and the counters.

python tools/substrings_bench.py [--out DIR] [--calls K] [--only NAME,...] [--mib M]
Writes DIR/substrings_table.txt (default DIR: profiles/).  Every answer is checked on samples: the rows' substrings are compared
in the text at the first and the last occurrence, and the ranked keys must not increase."""
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

SORT_CLASSES = ("k_radix_upsweep", "k_onesweep")
QUERIES = (("all_min50", dict(min_len=50, max_len=0, min_count=2, order=sa.SUBSTR_ALL, k=0)),
           ("cover_k65536_max16", dict(min_len=1, max_len=16, min_count=2, order=sa.SUBSTR_BY_COVER, k=65536)))


def workloads(mib):
    n = mib << 20
    return {"english_%dm" % mib: lambda: corpus.workload("c3_english_256m", n_override=n),
            "dna_%dm" % mib: lambda: corpus.dna(n, 4)}


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
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            xs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(xs), max(xs) - min(xs)


def sampled_ok(t, arr, rows, pos, q, samples=200):
    if rows.shape[0] == 0:
        return True
    rng = np.random.default_rng(1)
    for r in rng.integers(0, rows.shape[0], samples):
        lo, count, depth, parent = (int(x) for x in rows[r])
        if not (count >= max(2, q["min_count"]) and parent < depth and depth >= q["min_len"] and int(arr[lo]) == int(pos[r])):
            return False
        a, b, m = int(arr[lo]), int(arr[lo + count - 1]), min(depth, 4096)
        if not (np.array_equal(t[a:a + m], t[b:b + m]) and np.array_equal(t[a + depth - m:a + depth], t[b + depth - m:b + depth])):
            return False
        if a + depth < t.size and b + depth < t.size and count == 2 and t[a + depth] == t[b + depth]:      # the node ends at depth
            return False
    if q["order"] == sa.SUBSTR_BY_COVER:
        key = rows[:, 1].astype(np.int64) * np.minimum(rows[:, 2].astype(np.int64), q["max_len"] or (1 << 40))
        return bool((np.diff(key) <= 0).all())
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--mib", type=int, default=256)
    args = ap.parse_args()
    hdr = ("workload", "query", "n", "substrings_ms", "spread_ms", "lcp_ms", "substrings_over_lcp", "sa_build_ms", "lcp_inside_ms", "nsv_ms",
           "passes_ms", "sort_ms", "total", "nodes", "selected", "distinct_all", "distinct_selected", "unresolved_share",
           "steps_per_unresolved", "far_max", "select_passes", "sorted", "readbacks", "check")
    lines = []
    for name, make in workloads(args.mib).items():
        if args.only and name not in args.only.split(","):
            continue
        t = np.ascontiguousarray(make())
        n = t.size
        dT = torch.from_numpy(t).to("cuda")
        dS = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        wsa, wl, ws = sa.workspace_bytes(n), sa.lcp_work_bytes(n), sa.substrings_work_bytes(n)
        dW = torch.empty(max(wsa, wl, ws), dtype=torch.uint8, device="cuda")
        dL = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        cap = 1 << 24
        dR = torch.empty(4 * cap, dtype=torch.int32, device="cuda")
        dP = torch.empty(cap, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sm, _ = timed(lambda: sa.saca_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dW.data_ptr(), wsa), args.calls)

        def lcp_call():
            sa.lcp_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dL.data_ptr(), dW.data_ptr(), wl)
        lm, _ = timed(lcp_call, args.calls)
        lcp_classes = class_ms(lcp_call)
        arr = dS.cpu().numpy().view(np.uint32)
        for qname, q in QUERIES:
            query = sa.SubstrQuery(q["min_len"], q["max_len"], q["min_count"], q["order"], q["k"])
            total = []

            def sub_call():
                total.append(sa.substrings_device_ptr(dT.data_ptr(), dS.data_ptr(), n, query, dR.data_ptr(), dP.data_ptr(), cap, dW.data_ptr(), ws))
            zm, zsp = timed(sub_call, args.calls)
            st = sa.last_substr_stats()
            cls = class_ms(sub_call)
            wrote = min(total[-1], cap)
            rows = dR[:4 * wrote].cpu().numpy().view(np.uint32).reshape(-1, 4)
            pos = dP[:wrote].cpu().numpy().view(np.uint32)
            inside = sum(lcp_classes.values())
            nsv = cls.get("k_lcp_phi", 0.0) - lcp_classes.get("k_lcp_phi", 0.0)
            sort = sum(cls.get(k, 0.0) - lcp_classes.get(k, 0.0) for k in SORT_CLASSES)
            row = (name, qname, n, round(zm, 2), round(zsp, 2), round(lm, 2), round(zm / lm, 2), round(sm, 2), round(inside, 2), round(nsv, 2),
                   round(cls.get("k_rep_spans", 0.0), 2), round(sort, 2), total[-1], st["nodes"], st["selected"], st["distinct_all"],
                   st["distinct_selected"], round(st["unresolved"] / n, 4), round(st["far_steps"] / max(st["unresolved"], 1), 1), st["far_max"],
                   st["select_passes"], st["sorted"], st["readbacks"], "sampled" if sampled_ok(t, arr, rows, pos, q) else "MISMATCH")
            lines.append("  ".join(f"{h}={v}" for h, v in zip(hdr, row)))
            print(lines[-1], flush=True)
        del dT, dS, dL, dR, dP, dW, arr
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "substrings_table.txt"), "w") as f:
        f.write(f"tools/substrings_bench.py  ({torch.cuda.get_device_name(0)}; median and spread of {args.calls} calls after one warm-up, each ending in "
                "a device synchronise; array resident; lcp_ms = sa_amd_lcp_device on the same text in the same run; *_ms stage columns: HIP-event "
                "time of one more call -- lcp_inside_ms all classes of the LCP call, nsv_ms and sort_ms the classes k_lcp_phi and k_radix_upsweep + "
                "k_onesweep less the LCP call's share, passes_ms the class k_rep_spans)\n")
        for ln in lines:
            f.write(ln + "\n")
    return 0 if all("MISMATCH" not in ln for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
