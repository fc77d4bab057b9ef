"""What the refused-allocation tests share (no test in here, and on purpose no conftest: nothing of it reaches another module).

The contract ("Refused allocations"): a memory request the runtime refuses is SA_AMD_ENOMEM with nothing
written -- or a documented fallback with the same answers -- and leaves neither a pending runtime error, nor a changed index, nor
a leaked block behind.

  Abi             every function of the interface headers with a prototype made from its declaration (pointers as void *), on a
                  ctypes handle of its own: the wrapper raises on a non-zero code, so the cases call the library themselves.
                  Which parameters are OUTPUTS is read from the declaration too: a pointer that is not const (the index under
                  change, the work block, the stream and the statistics apart)
  Hooks           the refusal switch and the ledger of the diagnostic library (sa_amd_debug_refuse_alloc and its getters,
                  sa_amd_debug_live_allocations: csrc/sa_diag.h)
  on_a_fresh_thread  runs a function on a thread of its own: the switch, the pinned read-back block and its `failed` flag, the
                  per-thread knobs and the runtime's last error are thread_local, born and gone with the case"""
import ctypes
import re
import threading

import numpy as np

import suffix_array_amd as sa
import test_streams as ts

OK, ENOMEM = 0, -2                      # SA_AMD_OK, SA_AMD_ENOMEM
KIND_NAMES = {1: "device", 2: "pinned", 3: "table"}      # the seams: ResourcePool::acquire, ResourcePool::pinned, DevBuf::alloc
NOT_AN_OUTPUT = ("stream", "dWork", "stats")             # pointers without const that a call does not answer in
CANARY, HOST_CANARY = ts.CANARY, ts.HOST_CANARY      # the byte of an output array; what a host word (one int64) holds before the call
CTYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "void": None}


def declarations():
    """fn -> (return type, [(type, name, is a pointer, is an output)]) of every declaration of the interface headers"""
    out = {}
    for text in ts.interface_headers().values():
        for ret, fn, params in re.findall(r"\b(int32_t|int64_t|void|const char \*)\s*(sa_amd_\w+)\s*\(([^;{}()]*)\)\s*;", text):
            plist = []
            for k, p in enumerate(p for p in (re.sub(r"\s+", " ", x).strip() for x in params.split(",")) if p and p != "void"):
                m = re.fullmatch(r"(.*?)(\w+)", p)
                typ, name = m.group(1).strip(), m.group(2)
                pointer = "*" in typ
                handle = k == 0 and name == "ix"
                output = pointer and not typ.startswith("const ") and "*const" not in typ and name not in NOT_AN_OUTPUT and not handle
                plist.append((typ, name, pointer, output))
            out[fn] = (ret, plist)
    return out


class Abi:
    """the library at `path` (already in the process) with prototypes of its own"""

    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        self.decl = declarations()
        for fn, (ret, plist) in self.decl.items():
            f = getattr(self.L, fn)
            f.argtypes = [ctypes.c_void_p if pointer else CTYPES[typ] for typ, _, pointer, _ in plist]
            f.restype = ctypes.c_char_p if "char" in ret else CTYPES[ret]

    def outputs(self, fn, args):
        """the arrays among `args` (name -> value, in the declaration's order) that the call answers in"""
        plist = self.decl[fn][1]
        assert [name for _, name, _, _ in plist] == list(args), (fn, list(args))
        return {name: args[name] for _, name, _, output in plist if output and args[name] is not None}

    def call(self, fn, args):
        return getattr(self.L, fn)(*[as_argument(v) for v in args.values()])


def as_argument(v):
    if isinstance(v, np.ndarray):
        assert v.flags.c_contiguous
        return v.ctypes.data
    if isinstance(v, ctypes.Structure):
        return ctypes.addressof(v)
    if hasattr(v, "_h"):                                              # an index of the wrapper: its handle
        return v._h
    return v


def is_host_word(a):
    return a.dtype == np.int64 and a.size == 1


def fill_canary(outputs):
    for a in outputs.values():
        assert isinstance(a, np.ndarray) and a.flags.writeable, "an output is a numpy array of the case's own"
        if is_host_word(a):
            a[0] = HOST_CANARY
        else:
            a.view(np.uint8).reshape(-1)[:] = CANARY


def untouched(a):
    return int(a[0]) == HOST_CANARY if is_host_word(a) else bool(np.all(a.view(np.uint8) == CANARY))


def out(count, dtype=np.uint32):
    """an output array (the driver fills it with the canary)"""
    return np.zeros(int(count), dtype=dtype)


class Hooks:
    def __init__(self, abi):
        L = abi.L
        L.sa_amd_debug_refuse_alloc.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_refuse_alloc.restype = ctypes.c_int32
        L.sa_amd_debug_refuse_fired.argtypes = []
        L.sa_amd_debug_refuse_fired.restype = ctypes.c_int32
        L.sa_amd_debug_refuse_kinds.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        L.sa_amd_debug_refuse_kinds.restype = ctypes.c_int32
        L.sa_amd_debug_live_allocations.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.sa_amd_debug_live_allocations.restype = ctypes.c_int32
        self.L = L

    def refuse(self, nth):
        """arms the calling thread's switch (0: count only, -1: off); the requests since it was last set"""
        return int(self.L.sa_amd_debug_refuse_alloc(nth))

    def fired(self):
        return int(self.L.sa_amd_debug_refuse_fired())

    def kinds(self):
        """the kinds of the requests counted since the calling thread last set the switch"""
        buf = np.zeros(64, dtype=np.uint8)
        made = int(self.L.sa_amd_debug_refuse_kinds(buf.ctypes.data, buf.size))
        assert 0 <= made <= 64, made
        return tuple(KIND_NAMES[int(k)] for k in buf[:made])

    def ledger(self):
        """(live device allocations, live pinned blocks) made through the seams, process-wide"""
        dev, pin = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert self.L.sa_amd_debug_live_allocations(ctypes.addressof(dev), ctypes.addressof(pin)) == OK
        return int(dev.value), int(pin.value)


def on_a_fresh_thread(fn):
    """fn() on a new thread; what it returns, or what it raised"""
    box = {}

    def work():
        try:
            box["value"] = fn()
        except BaseException as e:                                    # noqa: B902 -- handed to the caller's thread
            box["error"] = e
    t = threading.Thread(target=work)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def pattern_batch(pats, dtype=np.uint8):
    """(pat_data, pat_off, count) as the ABI takes them"""
    if dtype == np.uint8:
        return sa._pattern_batch(pats)
    arrays = [np.asarray(p, dtype=dtype) for p in pats]
    return sa._batch_of(arrays, dtype)
