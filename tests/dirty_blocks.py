"""What the dirty-block tests share (no test in here, and on purpose no conftest: nothing of it reaches another module).

The contract ("Pooled-block scope"): no result and no statistic depends on the bytes a work block, a
table's allocation or the slack behind an input held before the call.

  PATTERNS        the five states of a recycled block the tests put there, in the order the GPU runs take them: zero and
                  small first, because a stale read under them is a wrong answer and no wild address
  fill_bytes      the pattern as bytes, for the blocks a caller brings (tests/test_dirty_work_blocks.py)
  diag_library    points the Python wrapper at libsuffix_array_amd_diag.so, whose fill switch (sa_amd_debug_fill_blocks,
                  csrc/sa_diag.h) does the same to the blocks the library takes itself (tests/test_dirty_blocks.py)"""
import contextlib
import ctypes
import gc

import numpy as np

import suffix_array_amd as sa

DIAG_LIB_NAME = "libsuffix_array_amd_diag.so"
FILL_OFF, FILL_SMALL, FILL_RANDOM = -1, 256, 257
PATTERNS = {"zero": 0x00, "small": FILL_SMALL, "random": FILL_RANDOM, "a5": 0xA5, "ff": 0xFF}
ORDER = tuple(PATTERNS)


def mix(x):
    """a fixed 32-bit integer hash (the one of csrc/host/support.hpp; any would do)"""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def fill_bytes(pattern, size, seed=0):
    """`size` bytes of the pattern: a byte value everywhere, or 32-bit word i = mix(i + seed) (% 5 for "small")"""
    code = PATTERNS[pattern]
    if code < FILL_SMALL:
        return np.full(size, code, dtype=np.uint8)
    words = mix(np.arange((size + 3) // 4, dtype=np.uint64) + seed)
    if code == FILL_SMALL:
        words %= 5
    return words.view(np.uint8)[:size].copy()


class DiagLibrary:
    """the diagnostic library while the wrapper points at it; the indexes made through it are tracked, so that none outlives it"""

    def __init__(self, L):
        self.L = L
        self._made = []

    def fill(self, pattern):
        """switches the fill to `pattern` (a name of PATTERNS, or None: off); returns the previous code"""
        return int(self.L.sa_amd_debug_fill_blocks(FILL_OFF if pattern is None else PATTERNS[pattern]))

    def _track(self, ix):
        assert ix._lib is self.L and sa.lib() is self.L, "an index of the diagnostic library made while the wrapper points elsewhere"
        self._made.append(ix)
        return ix

    def index(self, s, arr=None):
        return self._track(sa.DeviceIndex(s, arr))

    def token_index(self, tokens, arr=None):
        return self._track(sa.TokenIndex(tokens, arr))

    def close_all(self):
        for ix in self._made:
            assert ix._lib is self.L
            ix.close()
        self._made.clear()


@contextlib.contextmanager
def diag_library():
    """Inside, `sa.lib()` is the diagnostic library with every argtype of the product (it exports all of sa_amd_*), so the tests
    reach its routes through the ordinary wrapper.  No object made under one library is used under the other: what is
    unreachable is collected before either switch (an index destroys its handle through the library that made it), the indexes
    made through the DiagLibrary are closed on the way out, and the product library object comes back as it was."""
    gc.collect()
    product_name, product = sa._LIB_NAME, sa._lib
    sa._LIB_NAME, sa._lib = DIAG_LIB_NAME, None
    d = None
    try:
        L = sa.lib()
        L.sa_amd_debug_fill_blocks.argtypes = [ctypes.c_int32]
        L.sa_amd_debug_fill_blocks.restype = ctypes.c_int32
        L.sa_amd_release_cache.argtypes = []
        L.sa_amd_release_cache.restype = None
        assert product is None or L._handle != product._handle
        d = DiagLibrary(L)
        yield d
    finally:
        if d is not None:
            d.close_all()
            d.L.sa_amd_debug_fill_blocks(FILL_OFF)
            d.L.sa_amd_release_cache()
        gc.collect()
        sa._LIB_NAME, sa._lib = product_name, product
