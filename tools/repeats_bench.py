"""Repeat-finding timing: per workload of tools/lcp_bench.py, on device-resident text + suffix array,
sa_amd_lcp_device (the yardstick), sa_amd_repeat_lengths_device and sa_amd_repeat_spans_device in both modes at min_len 50; and
end to end from host pointers, sa_amd_repeat_spans with SA == NULL beside sa_amd_saca_u8_lcp plus the numpy definition on the host.

python tools/repeats_bench.py [--out DIR] [--calls K] [--only NAME,...] [--no-host] [--min-len K]
Writes DIR/r08_repeats_table.txt and DIR/r08_repeats_table.csv (default DIR: profiles/).  Every column, the host-pointer ones
included, is the median of K calls (default 5) after one warm-up, each ending in a device synchronise.  Every span list is checked
against the numpy definition over the downloaded arrays."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import suffix_array_amd as sa
from lcp_bench import WORKLOADS
from test_repeats_abi import keep_first_definition, repeat_lengths_definition, spans_definition


def timed(calls, fn):
    ms = []
    for k in range(calls + 1):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), max(ms) - min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--min-len", type=int, default=50)
    ap.add_argument("--no-host", action="store_true", help="skip the host-pointer end-to-end rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("repeats_bench: no GPU visible (timings are taken on the device only)")
    names = [k for k in WORKLOADS if not args.only or k in args.only.split(",")]
    k = args.min_len
    hdr = ("workload", "n", "lcp_ms", "lr_ms", "lr_spread_ms", "lr_over_lcp", "spans_all_ms", "spans_keep_first_ms", "spans_all",
           "spans_keep_first", "covered_all", "covered_keep_first", "host_spans_ms", "host_saca_lcp_numpy_ms", "check")
    rows = []
    for name in names:
        t = np.ascontiguousarray(WORKLOADS[name]())
        n = t.size
        dT = torch.from_numpy(t).to("cuda")
        dS = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        dL = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        cap = sa.repeat_spans_bound(n, k)
        dP = torch.empty(2 * cap + 2, dtype=torch.int32, device="cuda")
        wsa, wl, wr = sa.workspace_bytes(n), sa.lcp_work_bytes(n), sa.repeats_work_bytes(n)
        dW = torch.empty(max(wsa, wl, wr), dtype=torch.uint8, device="cuda")
        sa.saca_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dW.data_ptr(), wsa)
        torch.cuda.synchronize()
        lcp_ms, _ = timed(args.calls, lambda: sa.lcp_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dL.data_ptr(), dW.data_ptr(), wl))
        arr = dS.cpu().numpy().view(np.uint32)
        lcp = dL.cpu().numpy().view(np.uint32)
        lr_ms, lr_sp = timed(args.calls, lambda: sa.repeat_lengths_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dL.data_ptr(), dW.data_ptr(), wr))
        lr = dL.cpu().numpy().view(np.uint32)[:n]
        ok = np.array_equal(lr, repeat_lengths_definition(t, arr, lcp))
        res = {}
        for mode in (sa.REPEATS_ALL, sa.REPEATS_KEEP_FIRST):
            cnt = [0]

            def run():
                cnt[0] = sa.repeat_spans_device_ptr(dT.data_ptr(), dS.data_ptr(), n, k, mode, dP.data_ptr(), cap, dW.data_ptr(), wr)
            ms, _ = timed(args.calls, run)
            st = sa.last_repeat_stats()
            got = dP.cpu().numpy().view(np.uint32)[:2 * cnt[0]].reshape(-1, 2)
            exp = (keep_first_definition(t, arr, lcp, k) if mode else spans_definition(lr, k))[0]
            ok = ok and np.array_equal(got, exp)
            res[mode] = (ms, cnt[0], st["covered_bytes"])
        del dT, dS, dL, dP, dW
        torch.cuda.empty_cache()
        host_ms = ref_ms = float("nan")
        if not args.no_host:
            box = {}

            def host_spans():
                box["h"] = sa.repeat_spans(t, k, keep_first=True)

            def host_ref():
                a2, l2 = sa.saca_lcp(t)
                box["r"] = keep_first_definition(t, a2, l2, k)[0]
            host_ms, _ = timed(args.calls, host_spans)
            ref_ms, _ = timed(args.calls, host_ref)
            ok = ok and np.array_equal(box["h"], box["r"])
            sa.lib().sa_amd_release_cache()
        row = (name, n, round(lcp_ms, 2), round(lr_ms, 2), round(lr_sp, 2), round(lr_ms / lcp_ms, 2), round(res[0][0], 2), round(res[1][0], 2),
               res[0][1], res[1][1], res[0][2], res[1][2], round(host_ms, 1), round(ref_ms, 1), "definition" if ok else "MISMATCH")
        rows.append(row)
        print("  ".join(f"{h}={v}" for h, v in zip(hdr, row)), flush=True)
        del arr, lcp, lr, t
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "r08_repeats_table.csv"), "w") as f:
        f.write(",".join(hdr) + "\n")
        for r in rows:
            f.write(",".join(str(v) for v in r) + "\n")
    with open(os.path.join(args.out, "r08_repeats_table.txt"), "w") as f:
        f.write(f"tools/repeats_bench.py  ({torch.cuda.get_device_name(0)}; median of {args.calls} calls after one warm-up, each ending in a "
                f"device synchronise; min_len {k}; lcp = sa_amd_lcp_device on the same buffers; host spans = sa_amd_repeat_spans, KEEP_FIRST, "
                "SA == NULL, from host pointers; host ref = sa_amd_saca_u8_lcp + the numpy KEEP_FIRST definition on the host; both by the same method)\n")
        f.write(f"{'workload':20s} {'n':>11s} {'lcp ms':>8s} {'LR ms':>8s} {'+-':>6s} {'LR/lcp':>6s} {'ALL ms':>8s} {'KEEP ms':>8s} {'spans ALL':>10s} "
                f"{'spans KEEP':>10s} {'covered ALL':>12s} {'covered KEEP':>12s} {'host spans':>10s} {'host ref':>10s} check\n")
        for r in rows:
            f.write(f"{r[0]:20s} {r[1]:>11d} {r[2]:>8.2f} {r[3]:>8.2f} {r[4]:>6.2f} {r[5]:>6.2f} {r[6]:>8.2f} {r[7]:>8.2f} {r[8]:>10d} {r[9]:>10d} "
                    f"{r[10]:>12d} {r[11]:>12d} {r[12]:>10.1f} {r[13]:>10.1f} {r[14]}\n")
    return 0 if all(r[-1] != "MISMATCH" for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
