"""Burrows-Wheeler transform timing: sa_amd_bwt_device and sa_amd_unbwt_device on device-resident data,
per workload, beside the suffix-array build of the same text; the inverse's counters and its split over the kernel classes; the
host-pointer calls end to end beside sa_amd_saca_u8; the splitter spacing S swept on the corpus text; and the plain psi walk on
one CPU core (tools/psi_walk.c, compiled here) as a yardstick.

python tools/bwt_bench.py [--out DIR] [--calls K] [--only NAME,...] [--no-host] [--no-cpu]
Writes DIR/r07_bwt_table.txt (default DIR: profiles/).  Every result is checked: the round trip must give the text back, and the
forward transform is compared at 2 000 sampled rows with the text and the array on the host."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import suffix_array_amd as sa
from suffix_array_amd import corpus


def fib(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return np.frombuffer(b[:n], dtype=np.uint8).copy()


M256 = 256 << 20
WORKLOADS = {
    "c3_english_256m": lambda: corpus.workload("c3_english_256m"),
    "c2_uniform_256m": lambda: corpus.workload("c2_uniform_256m"),
    "c4_dna_1g": lambda: corpus.workload("c4_dna_1g"),
    "text_twice_256m": lambda: np.concatenate([corpus.english(M256 // 2, 5)] * 2),
    "fibonacci_256m": lambda: fib(M256),
}
KERNELS = ("k_bwt_gather", "k_onesweep32", "k_radix_upsweep32", "misc", "k_unbwt_walk", "k_unbwt_rank", "k_unbwt_write")


def timed(fn, calls):
    out = []
    for k in range(calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    names = [k for k in WORKLOADS if not args.only or k in args.only.split(",")]
    lines = [f"tools/bwt_bench.py --calls {args.calls}  ({torch.cuda.get_device_name(0)}; median (min..max) of {args.calls} calls after one "
             "warm-up, each ending in a device synchronise; fwd GB/s = 6 n bytes of compulsory traffic / forward time)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    ok = True
    for name in names:
        t = np.ascontiguousarray(WORKLOADS[name]())
        n = t.size
        dT = torch.from_numpy(t).to("cuda")
        dS = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        dB = torch.empty(n, dtype=torch.uint8, device="cuda")
        dO = torch.empty(n, dtype=torch.uint8, device="cuda")
        wsa, wu = sa.workspace_bytes(n), sa.unbwt_work_bytes(n)
        dW = torch.empty(max(wsa, wu), dtype=torch.uint8, device="cuda")
        prim = [0]
        sa_ms = timed(lambda: sa.saca_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dW.data_ptr(), wsa), args.calls)

        def fwd():
            prim[0] = sa.bwt_device_ptr(dT.data_ptr(), dS.data_ptr(), n, dB.data_ptr(), dW.data_ptr(), 256)

        def inv():
            sa.unbwt_device_ptr(dB.data_ptr(), n, prim[0], dO.data_ptr(), dW.data_ptr(), wu)

        f_ms = timed(fwd, args.calls)
        i_ms = timed(inv, args.calls)
        st = sa.last_unbwt_stats()
        good = bool(torch.equal(dO, dT))
        arr = dS.cpu().numpy().view(np.uint32)
        b = dB.cpu().numpy()
        rows = np.random.default_rng(1).integers(0, n, 2000)
        good = good and np.array_equal(b[rows], t[arr[rows + (rows >= prim[0])].astype(np.int64) - 1]) and int(arr[prim[0]]) == 0
        ok = ok and good
        emit(f"{name}: n={n} sa_build_ms={sa_ms[0]:.2f} ({sa_ms[1]:.2f}..{sa_ms[2]:.2f})  bwt_ms={f_ms[0]:.2f} ({f_ms[1]:.2f}..{f_ms[2]:.2f}) "
             f"fwd_GBps={6 * n / (f_ms[0] * 1e6):.0f}  unbwt_ms={i_ms[0]:.2f} ({i_ms[1]:.2f}..{i_ms[2]:.2f})  {st}  check={'ok' if good else 'MISMATCH'}")
        emit(f"{name}: forward kernels {kernel_split(fwd)}")
        emit(f"{name}: inverse kernels (ms, launches) {kernel_split(inv)}")
        if name == "c3_english_256m":
            for spacing in (64, 256, 1024):
                sa.unbwt_set_splitter_spacing(spacing)
                s_ms = timed(inv, args.calls)
                st = sa.last_unbwt_stats()
                emit(f"{name}: S={spacing} unbwt_ms={s_ms[0]:.2f} ({s_ms[1]:.2f}..{s_ms[2]:.2f}) walkers={st['walkers']} longest={st['longest_walk']} "
                     f"round trip {'ok' if torch.equal(dO, dT) else 'MISMATCH'}  {kernel_split(inv)}")
            sa.unbwt_set_splitter_spacing(-1)
            if not args.no_cpu:
                m = 64 << 20
                tb, tp = sa.bwt(t[:m])
                with tempfile.TemporaryDirectory() as tmp:
                    exe, path = os.path.join(tmp, "psi_walk"), os.path.join(tmp, "b.bin")
                    subprocess.check_call(["gcc", "-O2", "-o", exe, os.path.join(ROOT, "tools", "psi_walk.c")])
                    tb.tofile(path)
                    emit(f"{name}[:64 MiB] on ONE CPU core (tools/psi_walk.c; counting sort, then the plain walk): "
                         + subprocess.check_output([exe, path, str(tp)], text=True).strip())
        del dS, dB, dO, dW, dT, arr
        torch.cuda.empty_cache()
        if not args.no_host and n <= M256:
            out = np.empty(n + 1, dtype=np.uint32)
            a, c = [], []
            for k in range(args.calls + 1):
                t0 = time.perf_counter(); sa.saca(t, out); x = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter(); hb, hp = sa.bwt(t); y = (time.perf_counter() - t0) * 1e3
                if k:
                    a.append(x); c.append(y)
            good = hp == prim[0] and np.array_equal(hb, b)
            ok = ok and good
            emit(f"{name}: host pointers end to end: sa_amd_saca_u8 {statistics.median(a):.1f} ms ({min(a):.1f}..{max(a):.1f}); "
                 f"sa_amd_bwt(SA = NULL) {statistics.median(c):.1f} ms ({min(c):.1f}..{max(c):.1f})  check={'ok' if good else 'MISMATCH'}")
            del out, hb
            sa.lib().sa_amd_release_cache()
        del t, b
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "r07_bwt_table.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
