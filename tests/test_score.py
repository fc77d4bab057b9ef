"""GPU suite for scoring a text under the infinity-gram model: sa_amd_index_infgram_score compared bit for bit with
score_definition of tests/test_score_abi.py (checked against brute force there) and with the device's own sa_amd_index_infgram
on the explicit prompts, canaries around every output, every output NULL in turn, every group cap and table combination, the
statistics against that file's models of the gallop, of the long decision and of the work bounds.

Sizes: texts up to 256 KiB, queries up to 8 KiB; positions are 64-bit in the kernels and bounded by m < 2^31 on the long list."""
import functools
import subprocess
import sys
import threading

import numpy as np
import pytest

import suffix_array_amd as sa
from suffix_array_amd import corpus
from conftest import ROOT, fibonacci_word
from test_docs import same_for_every_route
from test_docs_abi import _u8
from test_ngram_abi import EXAMPLE_TEXT, ceil_log2
from test_score_abi import (NAMES, compared_bytes_bound, doc_starts, effective_group_cap, gallop_bound, gallop_model, predicted_long_positions,
                            score_definition)

pytestmark = pytest.mark.gpu

FILL32 = 0xA5A5A5A5
PAD = 32
CAPS = (0, 4, 64, 4096)


# ---------------------------------------------------------------- the calls ----

def raw_score(ix, qb, q_off, min_count, max_len, null=()):
    """sa_amd_index_infgram_score on numpy buffers with canaries around every output; the outputs named in `null` are passed as
    NULL -> dict of what was written (None for a NULL output) and the statistics"""
    q = _u8(qb)
    m = q.size
    bufs = {k: np.full(m + 2 * PAD, 0xA5 if k == "at_end" else FILL32, dtype=np.uint8 if k == "at_end" else np.uint32) for k in NAMES}
    fill = {k: v[0].copy() for k, v in bufs.items()}
    off = None if q_off is None else np.ascontiguousarray(q_off, dtype=np.int64)
    args = [None if k in null else bufs[k][PAD:].ctypes.data for k in NAMES]
    rc = sa.lib().sa_amd_index_infgram_score(ix._h, q.ctypes.data if m else None, m, None if off is None else off.ctypes.data,
                                             0 if off is None else off.size - 1, min_count, max_len, *args)
    assert rc == 0, rc
    out = {"stats": sa.last_score_stats()}
    for k, buf in bufs.items():                                       # nothing before, nothing behind, nothing at all through NULL
        w = 0 if k in null else m
        assert np.all(buf[:PAD] == fill[k]) and np.all(buf[PAD + w:] == fill[k]), k
        out[k] = None if k in null else buf[PAD:PAD + m].astype(np.int64)
    return out


@functools.lru_cache(maxsize=None)
def _definition(key, min_count, max_len):
    tb, arr, qb, q_off = _CASE[key]
    d = score_definition(tb, arr, qb, None if q_off is None else np.array(q_off), min_count, max_len)
    for v in d.values():
        v.setflags(write=False)
    return d


_CASE = {}


def definition(tb, arr, qb, q_off, min_count, max_len):
    """score_definition, computed once per case and shared"""
    key = (hash(tb), len(tb), qb, None if q_off is None else tuple(int(x) for x in q_off))
    _CASE.setdefault(key, (tb, arr, qb, None if q_off is None else tuple(int(x) for x in q_off)))
    return _definition(key, min_count, max_len)


def check_stats(st, d, n, m, q_off, min_count, max_len, cap):
    """the statistics against the models: exact where the model is, inside the bound where it is a bound"""
    ge = effective_group_cap(cap, max_len)
    start = doc_starts(m, q_off)
    group, long_, longs, probes = [], [], 0, 0
    for j in range(m):
        s = int(d["s"][j])
        _, g, l, is_long = gallop_model(lambda x: x <= s, min(j - int(start[j]), max_len), ge)
        group += g
        long_ += l
        longs += is_long
        probes += gallop_bound(s)
    assert longs == predicted_long_positions(m, q_off, d["s"], max_len, cap)
    want = {"positions": m, "documents": 1 if q_off is None else len(q_off) - 1, "group_cap": ge, "long_positions": longs,
            "zero_positions": int(np.count_nonzero(d["nhi"] == d["nlo"])), "group_searches": len(group), "long_searches": len(long_),
            "readbacks": (1 + (longs > 0)) if m else 0}
    assert {k: st[k] for k in want} == want, (st, want)
    assert st["range_searches"] == len(group) + len(long_) <= probes
    assert st["readbacks"] <= 2
    assert 0 <= st["compared_bytes"] <= compared_bytes_bound(n, group, long_), st
    assert 0 <= st["next_lookups"] <= 2 * m * (ceil_log2(n + 2) + 1)
    return longs


def check(ix, tb, arr, qb, q_off=None, min_count=1, max_len=sa.SCORE_MAX_CONTEXT, cap=-1, key=None, route=None, pin=True):
    """one call against the definition, its statistics against the models, and S / LO / HI / AT_END against the index's own
    infgram on the explicit prompts Q[max(start, j - max_len) .. j)"""
    d = definition(tb, arr, qb, q_off, min_count, max_len)
    prev = sa.score_set_group_cap(cap)
    try:
        got = raw_score(ix, qb, q_off, min_count, max_len)
    finally:
        sa.score_set_group_cap(prev)
    for k in NAMES:
        bad = np.flatnonzero(got[k] != d[k])[:4]
        assert bad.size == 0, (k, route, cap, min_count, max_len, [(int(j), int(got[k][j]), int(d[k][j])) for j in bad])
    m = len(qb)
    longs = check_stats(got["stats"], d, len(tb), m, q_off, min_count, max_len, cap)
    if pin and m:
        start = doc_starts(m, q_off)
        prompts = [qb[max(int(start[j]), j - max_len):j] for j in range(m)]
        s, lo, hi, ae = ix.infgram(prompts, min_count, max_len)[:4]
        for k, v in zip(NAMES[:4], (s, lo, hi, ae)):
            assert np.array_equal(got[k], v.astype(np.int64)), ("infgram", k, route)
    if key is not None:
        same_for_every_route(key, route, *(got[k] for k in NAMES))
    return got, longs


@functools.lru_cache(maxsize=None)
def text(kind):
    """-> (text bytes, suffix array): computed once, shared, never changed"""
    if kind == "english_256k":
        t = corpus.english_corpus(1 << 18, 5)
    elif kind == "english_8k":
        t = corpus.english_corpus(8192, 7)
    elif kind == "a_run":
        t = _u8(b"a" * 3000)
    elif kind == "period2":
        t = _u8(b"ab" * 1500)
    elif kind == "fibonacci":
        t = _u8(fibonacci_word(16)[:3000])
    else:
        raise KeyError(kind)
    from conftest import Oracle
    arr = Oracle().sais(t)
    arr.setflags(write=False)
    return t.tobytes(), arr


def substituted(qb, rate, seed):
    """the bytes with `rate` of them replaced by a value the English corpus does not hold"""
    rng = np.random.default_rng(seed)
    q = bytearray(qb)
    for j in rng.choice(len(q), max(1, int(len(q) * rate)), replace=False):
        q[int(j)] = 1 + int(rng.integers(0, 5))
    return bytes(q)


def index_of(kind, tables=()):
    tb, arr = text(kind)
    ix = sa.DeviceIndex(_u8(tb), arr)
    if "bkt" in tables:
        ix.buckets()
    if "lcp" in tables:
        ix.enable_lcp()
    return tb, arr, ix


# ---------------------------------------------------------------- the tests ----

def test_empty_text_empty_query_and_the_header_example(oracle):
    ix = sa.DeviceIndex(_u8(b""), oracle.sais(_u8(b"")))                # n = 0: one slot, every context but the empty one is absent
    got, _ = check(ix, b"", oracle.sais(_u8(b"")), b"abca", pin=False)
    assert not got["s"].any() and got["hi"].tolist() == [1] * 4 and got["nlo"].tolist() == got["nhi"].tolist() == [1] * 4
    ix.close()
    t = _u8(EXAMPLE_TEXT)
    arr = oracle.sais(t)
    ix = sa.DeviceIndex(t)                                             # the array is built on the device
    for cap in CAPS:
        got, _ = check(ix, EXAMPLE_TEXT, arr, b"xcabra", None, 1, 4, cap)
        assert [got[k].tolist() for k in NAMES] == [[0, 0, 1, 2, 2, 3], [0, 0, 8, 8, 2, 2], [12, 12, 9, 9, 4, 4], [1, 1, 0, 0, 0, 0],
                                                    [12, 8, 8, 8, 2, 2], [12, 9, 9, 8, 4, 4]]
        assert int(check(ix, EXAMPLE_TEXT, arr, b"xcabra", None, 3, 4, cap)[0]["s"][5]) == 0
    got = raw_score(ix, b"", None, 1, 4)                                # m = 0 succeeds and writes nothing
    assert got["stats"]["positions"] == 0 and got["stats"]["readbacks"] == 0 and got["s"].size == 0
    got = raw_score(ix, b"", [0, 0, 0], 1, 4)
    assert got["stats"]["documents"] == 2
    r = ix.infgram_score(b"xcabra", 1, 4)                              # the Python surface and its result object
    assert isinstance(r, sa.ScoreResult) and r.s.tolist() == [0, 0, 1, 2, 2, 3] and r.at_end.dtype == np.uint8 and r.nhi.dtype == np.uint32
    assert np.isneginf(r.log2_prob()[[0, 3]]).all() and r.log2_prob()[1] == pytest.approx(-np.log2(11.0))
    assert r.doc_bits([0, 2, 6])[1].tolist() == [1, 1]
    assert sa.SuffixArray(t).infgram_score(b"xcabra", max_len=4).nlo.tolist() == [12, 8, 8, 8, 2, 2]
    ix.close()


@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_query_lengths_around_the_tile(m):
    """slices of the text: the contexts reach back over the tile's start, into the staged halo (tile 0: into nothing)"""
    tb, arr, ix = index_of("english_256k")
    qb = substituted(tb[70001:70001 + m], 0.02, m)
    for cap in (-1, 4096):
        got, _ = check(ix, tb, arr, qb, cap=cap)
    assert int(got["s"].max()) > 20 and (m < 257 or int(got["s"][256:].max()) > 2)
    ix.close()


def test_document_starts_and_empty_documents():
    tb, arr, ix = index_of("english_256k")
    qb = tb[5000:5513]
    m = len(qb)
    tables = {"first of a tile": [0, 256, m], "last of a tile": [0, 255, 511, m], "mid tile": [0, 100, 300, 301, m],
              "empty documents": [0, 0, 0, 200, 200, 256, 256, 400, m, m, m], "every position": list(range(m + 1))}
    for name, off in tables.items():
        for cap in (-1, 4, 4096):
            got, _ = check(ix, tb, arr, qb, off, cap=cap, route=name)
        start = doc_starts(m, off)
        assert np.all(got["s"] <= np.arange(m) - start) and np.all(got["s"][np.isin(np.arange(m), off)] == 0), name
    one, _ = check(ix, tb, arr, qb, [0, m])                            # ndocs = 1 is q_off = NULL
    none, _ = check(ix, tb, arr, qb, None)
    assert all(np.array_equal(one[k], none[k]) for k in NAMES) and int(none["s"][-1]) == m - 1
    ix.close()


@pytest.mark.parametrize("max_len", [1, 2, 63, 64, 65, 4096])
def test_context_caps(max_len):
    tb, arr, ix = index_of("english_256k")
    qb = substituted(tb[123456:123456 + 600], 0.01, max_len)
    for cap in CAPS:
        got, _ = check(ix, tb, arr, qb, None, 1, max_len, cap, key=("max_len", max_len), route=cap)
    assert min(max_len, 65) <= int(got["s"].max()) <= max_len           # (six substitutions in 600 bytes leave a run of 84)
    ix.close()


def test_min_counts():
    tb, arr, ix = index_of("english_256k")
    n = len(tb)
    qb = substituted(tb[200000:200300], 0.02, 3)
    for min_count in (1, 2, n + 2):
        got, _ = check(ix, tb, arr, qb, None, min_count)
        assert np.all((got["s"] == 0) | (got["hi"] - got["lo"] >= min_count))
    assert not got["s"].any() and np.all(got["hi"] - got["lo"] == n + 1) and np.all(got["at_end"] == 1)    # n + 2: the unigram model everywhere
    ix.close()


def test_absent_byte_and_the_texts_last_bytes():
    tb, arr, ix = index_of("english_256k")
    assert 0xFF not in tb
    tail = 2000
    qb = tb[300:340] + b"\xff" + tb[340:360] + tb[-tail:] + b"\xff" + tb[-3:]
    got, _ = check(ix, tb, arr, qb, [0, 61, len(qb)])
    j = 40                                                             # the absent byte: nothing follows any context with it
    assert got["nhi"][j] == got["nlo"][j] == got["hi"][j] and got["s"][j + 1] == 0
    j = 61 + tail                                                      # the context is the text's last 2000 bytes and occurs only there
    assert (got["s"][j], got["at_end"][j], got["hi"][j] - got["lo"][j]) == (tail, 1, 1) and got["nhi"][j] == got["nlo"][j]
    r = ix.infgram_score(qb, doc_offsets=[0, 61, len(qb)])
    assert r.counts()[1][j] == 0 and np.isneginf(r.log2_prob()[j])     # denominator 0
    ix.close()


def test_the_text_itself_and_a_slice_with_substitutions():
    """query = T at 8 KiB with max_len = 4096 and 1 % substitutions: contexts of hundreds of bytes, the long path in use"""
    tb, arr, ix = index_of("english_8k")
    qb = substituted(tb, 0.01, 8)
    for cap in (-1, 0):
        got, longs = check(ix, tb, arr, qb, cap=cap, key="whole", route=cap, pin=cap < 0)
        assert longs > 0 and got["stats"]["long_positions"] == longs
    assert int(got["s"].max()) > 64 and np.count_nonzero(got["nhi"] == got["nlo"]) >= 40
    got, longs = check(ix, tb, arr, substituted(tb[1000:3000], 0.01, 9), [0, 700, 2000])
    assert longs > 0
    ix.close()


@pytest.mark.parametrize("kind", ["a_run", "period2", "fibonacci"])
def test_long_lcp_families(kind):
    tb, arr, ix = index_of(kind)
    qb = tb[:1100] + b"c" + tb[5:700]
    for cap, min_count in ((-1, 1), (0, 1), (4096, 2)):
        got, longs = check(ix, tb, arr, qb, None, min_count, 4096, cap, pin=cap < 0)
        assert min_count > 1 or (int(got["s"].max()) == 1100 and longs > 1000)
    ix.close()


@pytest.mark.parametrize("tables", [(), ("bkt",), ("lcp",), ("bkt", "lcp")], ids=["plain", "bkt", "lcp", "bkt_lcp"])
def test_answers_do_not_depend_on_the_route(tables):
    tb, arr, ix = index_of("english_256k", tables)
    qb = substituted(tb[40000:40700], 0.01, 5) + tb[-30:] + b"\xff" + tb[90000:90300]
    off = [0, 0, 300, 731, len(qb)]
    for cap in CAPS:
        for min_count, max_len in ((1, 4096), (2, 100)):
            check(ix, tb, arr, qb, off, min_count, max_len, cap, key=("routes", min_count, max_len), route=(tables, cap), pin=cap == 64)
    ix.close()


def test_every_output_may_be_null():
    tb, arr, ix = index_of("english_256k")
    qb = tb[1000:1300]
    d = definition(tb, arr, qb, None, 1, 4096)
    for name in NAMES:
        got = raw_score(ix, qb, None, 1, 4096, null=(name,))
        assert got[name] is None and all(np.array_equal(got[k], d[k]) for k in NAMES if k != name), name
    got = raw_score(ix, qb, None, 1, 4096, null=NAMES)                 # everything NULL: only the statistics
    assert got["stats"]["positions"] == len(qb) and got["stats"]["zero_positions"] == int(np.count_nonzero(d["nhi"] == d["nlo"]))
    ix.close()


def test_invalid_arguments_write_nothing():
    ix = sa.DeviceIndex(_u8(EXAMPLE_TEXT))
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    before = sa.last_score_stats()
    for off, ndocs, min_count, max_len, m in (([0, 4], 1, 0, 8, 4), ([0, 4], 1, 1, 0, 4), ([0, 4], 1, 1, 4097, 4), ([0, 3], 1, 1, 8, 4),
                                              ([1, 4], 1, 1, 8, 4), ([0, 3, 2, 4], 3, 1, 8, 4), ([0, 4], -1, 1, 8, 4), ([0, 4], 1, 1, 8, -1)):
        a = np.array(off, dtype=np.int64)
        assert L.sa_amd_index_infgram_score(ix._h, p, m, a.ctypes.data, ndocs, min_count, max_len, p, p, p, p, p, p) == -1, off
    assert np.all(buf == 0x77777777) and sa.last_score_stats() == before
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score(b"abc", max_len=0)
    with pytest.raises(sa.SuffixArrayError):
        ix.infgram_score(b"abc", doc_offsets=[0, 2])
    ix.close()


def test_an_array_that_is_no_suffix_array_is_survived():
    """a permutation of the right entries in the wrong order (every entry in range): the answers are unspecified; the calls
    return and write inside the outputs only"""
    tb, arr = text("english_8k")
    s = sa.SuffixArray.unchecked_from_parts(_u8(tb), np.random.default_rng(9).permutation(arr).astype(np.uint32))
    qb = substituted(tb[:1500], 0.01, 4)
    for tables in ((), ("bkt",)):
        if tables:
            s.enable_buckets()
        ix = s._index()
        for cap in CAPS:
            prev = sa.score_set_group_cap(cap)
            try:
                for min_count, max_len in ((1, 4096), (2, 7)):
                    raw_score(ix, qb, [0, 500, 1500], min_count, max_len)
            finally:
                sa.score_set_group_cap(prev)


_TORCH_CALLER = r'''
import sys
import numpy as np
import torch                                    # first: the process then has one HIP runtime, torch's
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import suffix_array_amd as sa
from suffix_array_amd import corpus
from test_score import NAMES, PAD, raw_score, substituted

tb = corpus.english_corpus(1 << 16, 5).tobytes()
ix = sa.DeviceIndex(np.frombuffer(tb, dtype=np.uint8))            # the array is built on the device
qb = substituted(tb[30000:31000], 0.01, 6) + tb[31000:31900]
m = len(qb)
off = [0, 10, 1000, m]
dev = torch.device("cuda", 0)
for cap, offset, q_off, null in ((-1, 0, None, ()), (4, 3, off, ("lo",)), (0, 1, off, ("s", "nhi"))):
    ndocs = 1 if q_off is None else len(q_off) - 1
    wb = sa.score_work_bytes(m, ndocs)
    assert wb >= 12 * m
    dq = torch.zeros(m + 16, dtype=torch.uint8, device=dev)
    dq[offset:offset + m] = torch.from_numpy(np.frombuffer(qb, dtype=np.uint8).copy()).to(dev)
    outs = {k: torch.full((m + 2 * PAD,), 0x25, dtype=torch.uint8 if k == "at_end" else torch.int32, device=dev) for k in NAMES}
    work = torch.empty(wb + 256, dtype=torch.uint8, device=dev)
    wp = (work.data_ptr() + 255) & ~255
    ptrs = [0 if k in null else outs[k].data_ptr() + PAD * outs[k].element_size() for k in NAMES]
    torch.cuda.synchronize()
    prev = sa.score_set_group_cap(cap)
    try:
        sa.infgram_score_device_ptr(ix, dq.data_ptr() + offset, m, 1, 4096, *ptrs, wp, wb, doc_offsets=q_off,
                                    stream=torch.cuda.current_stream().cuda_stream)
        st = sa.last_score_stats()
        host = raw_score(ix, qb, q_off, 1, 4096)
    finally:
        sa.score_set_group_cap(prev)
    assert st == host["stats"] and st["long_positions"] > 0, (st, host["stats"])
    assert int(host["s"].max()) > 64
    for k in NAMES:
        got = outs[k].cpu().numpy()
        w = 0 if k in null else m
        assert np.all(got[:PAD] == 0x25) and np.all(got[PAD + w:] == 0x25), k
        if k not in null:
            assert np.array_equal(got[PAD:PAD + m].astype(np.int64) & 0xFFFFFFFF, host[k]), k
try:                                                               # a work block that is too small is refused
    sa.infgram_score_device_ptr(ix, dq.data_ptr(), m, 1, 4096, 0, 0, 0, 0, 0, 0, wp, 256)
    raise SystemExit("a work block of 256 bytes was accepted")
except sa.SuffixArrayError:
    pass
ix.close()
print("ok")
'''


def test_device_form_on_torch_tensors(tmp_path):
    """sa_amd_index_infgram_score_device on torch tensors and torch's stream against the host form, in a process of its own:
    torch brings its own HIP runtime, which has to be the first one the process loads"""
    src = tmp_path / "score_torch_caller.py"
    src.write_text(_TORCH_CALLER)
    out = subprocess.run([sys.executable, str(src), ROOT], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_two_threads_with_different_group_caps():
    tb, arr, ix = index_of("english_8k")
    queries = [substituted(tb[100:2100], 0.01, 20 + j) for j in range(2)]
    defs = [definition(tb, arr, q, None, 1, 4096) for q in queries]
    caps = (0, 4096)
    errors = []

    def work(j):
        try:
            sa.score_set_group_cap(caps[j])                            # (the switch is the calling thread's)
            for _ in range(4):
                got = raw_score(ix, queries[j], None, 1, 4096)
                assert all(np.array_equal(got[k], defs[j][k]) for k in NAMES)
                assert got["stats"]["group_cap"] == caps[j] and got["stats"]["positions"] == len(queries[j])
                assert (got["stats"]["long_positions"] > 0) == (caps[j] == 0) and (got["stats"]["group_searches"] == 0) == (caps[j] == 0)
        except Exception as e:                                        # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert sa.score_set_group_cap(-1) == sa.SCORE_GROUP_CAP_DEFAULT    # the workers' switches were their own: this thread's is untouched
    ix.close()


def test_the_other_features_statistics_are_left_untouched():
    tb, arr, ix = index_of("english_8k", ("lcp",))
    ix.search([b"the", b"e"])
    ix.match_stats(tb[:100], 16)
    ix.infgram([tb[50:90], b"q"], 2)
    readers = (sa.last_search_stats, sa.last_ngram_stats, sa.last_match_stats, sa.last_lcp_stats, sa.last_stats)
    before = [f() for f in readers]
    ix.infgram_score(tb[:3000], 1, 4096)
    assert [f() for f in readers] == before
    st = sa.last_score_stats()
    assert st["positions"] == 3000 and st["long_positions"] > 0 and st["readbacks"] == 2
    ix.close()
