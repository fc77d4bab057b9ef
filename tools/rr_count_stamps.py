"""Diagnostic: in which step of its chain a workgroup of k_rr_count waits (s_memtime stamps of wave 0, C3; every stamp but
"loads issued" first waits for everything the wave has outstanding).  Ten launches per build: the set-up and the nine rounds, summed."""
import sys, os, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import suffix_array_amd as sa
from suffix_array_amd import corpus
t = corpus.workload(sys.argv[1] if len(sys.argv) > 1 else "c3_english_256m")
out = np.zeros(t.size + 1, dtype=np.uint32)
L = sa.diag_lib()        # the stamps are compiled into the diagnostic library only
saca = lambda text, arr: L.sa_amd_saca_u8(text.ctypes.data, arr.ctypes.data, text.size)
buf = (ctypes.c_uint64 * 16)()
assert saca(t, out) == 0
L.sa_amd_debug_rr_count_stamps(1)
L.sa_amd_debug_phase_cycles(buf, 16)          # zero
assert saca(t, out) == 0
L.sa_amd_debug_phase_cycles(buf, 16)
L.sa_amd_debug_rr_count_stamps(0)
names = ["byte loads of the span issued", "span classified (+ wait for the bytes and the keys of KEYED places)",
         "barrier (the slowest wave of the workgroup)", "wave reduction, the tile's look-up in U, stores"]
tot = sum(buf[i] for i in range(len(names)))
for i, nm in enumerate(names):
    print(f"{nm:72s} {100.0 * buf[i] / max(tot, 1):5.1f} %   {buf[i]}")
