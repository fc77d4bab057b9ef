#!/usr/bin/env python3
"""Work-block sizes of the C ABI at the sizes where a layout changes: python tools/work_bytes_table.py [libsuffix_array_amd.so]
Host-only (no GPU is touched).  The table is part of the ABI: run it on two builds and compare the output."""
import ctypes, os, sys

FUNCS = ["sa_amd_workspace_bytes", "sa_amd_lcp_work_bytes", "sa_amd_unbwt_work_bytes", "sa_amd_check_integrity_work_bytes",
         "sa_amd_repeats_work_bytes", "sa_amd_lz_work_bytes", "sa_amd_match_work_bytes", "sa_amd_docs_work_bytes"]
SIZES = [0, 1, 8191, 8192, 8193, (1 << 20) + 3, 1 << 25, (1 << 31) - 1]

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "suffix_array_amd", "libsuffix_array_amd.so")
L = ctypes.CDLL(path)
print("n " + " ".join(f.replace("sa_amd_", "").replace("_bytes", "") for f in FUNCS))
for n in SIZES:
    row = []
    for f in FUNCS:
        fn = getattr(L, f)
        fn.argtypes = [ctypes.c_int32]
        fn.restype = ctypes.c_int64
        row.append(str(fn(n)))
    print(f"{n} " + " ".join(row))
