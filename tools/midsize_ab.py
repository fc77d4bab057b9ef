"""1 MiB builds, host-pointer entry point measured as tools/midsize_timing.py does (sa.saca: best of 5 end to end and the library's
own build time), one process per library and leg, legs alternating.  python tools/midsize_ab.py LIB_A LIB_B LEGS   (file names inside suffix_array_amd/)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, time, statistics
sys.path.insert(0, sys.argv[1])
import numpy as np
import suffix_array_amd as sa
from suffix_array_amd import corpus
sa._LIB_NAME = sys.argv[2]
for gen in ("english_corpus", "uniform"):
    n = 1 << 20
    t = getattr(corpus, gen)(n, 3)
    out = np.zeros(n + 1, dtype=np.uint32)
    for _ in range(5):
        sa.saca(t, out)
    e2e, build = [], []
    for _ in range(200):
        t0 = time.perf_counter(); sa.saca(t, out); e2e.append((time.perf_counter() - t0) * 1e3)
        build.append(sa.last_host_timing()["build"])
    st = sa.last_stats()
    print(f"{sys.argv[2]:28s} {gen:15s} 1 MiB  200 calls: build median {statistics.median(build):.4f} min {min(build):.4f} ms   e2e median {statistics.median(e2e):.4f} best of first 5 {min(e2e[:5]):.4f} min {min(e2e):.4f} ms  rounds {st['rounds']} readbacks {st['readbacks']}", flush=True)
'''
a, b, legs = sys.argv[1], sys.argv[2], int(sys.argv[3])
for lib in (a, b) * legs:
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, lib], capture_output=True, text=True, timeout=200)
    if p.returncode != 0:
        print(lib, "FAILED", p.stderr[-800:]); sys.exit(1)
    print(p.stdout, end="", flush=True)
