"""CPU suite for document-aware duplicate spans: the run rule of include/suffix_array_amd.h restated in numpy over the oracle's
suffix array (vectorised, and once more as a plain loop over the runs) and checked against the literal double loop over
windows; the ndocs = 1 identities with the boundary-blind definitions of tests/test_repeats_abi.py; the exports, the Python
surface and the argument checks that answer without a device."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import suffix_array_amd as sa
from conftest import ROOT, adversarial_cases
from test_docs_abi import EXAMPLE_OFF, EXAMPLE_TEXT, offset_tables
from test_lcp_abi import _kasai
from test_repeats_abi import _u8, _union, intervals, keep_first_definition, repeat_lengths_definition, spans_definition

EXPORTS = ("sa_amd_doc_repeats_work_bytes", "sa_amd_index_doc_repeat_spans", "sa_amd_last_doc_repeat_stats")
ALL, KEEP_FIRST = sa.REPEATS_ALL, sa.REPEATS_KEEP_FIRST
ANY, OTHER = 0, 1
COMBOS = [(ALL, ANY), (ALL, OTHER), (KEEP_FIRST, ANY), (KEEP_FIRST, OTHER)]
BRUTE_LIMIT = 200                                                     # bytes up to which the literal double loop runs


# ---------------------------------------------------------------- the definitions ----

def answer_of(flagged, off, n, k, members):
    """spans, doc_bytes and the statistics that follow from the flagged positions"""
    flagged = np.asarray(flagged, dtype=np.int64)
    offa = np.asarray(off, dtype=np.int64)
    covered = _union(flagged, np.full(flagged.size, k, dtype=np.int64), n)
    spans = intervals(covered)
    c = np.concatenate([[0], np.cumsum(covered)])
    doc_bytes = c[offa[1:]] - c[offa[:-1]]
    stats = {"members": int(members), "flagged": int(flagged.size), "spans": int(spans.shape[0]), "covered_bytes": int(covered.sum()),
             "docs_touched": int(np.count_nonzero(doc_bytes))}
    assert int(doc_bytes.sum()) == stats["covered_bytes"]
    return {"flagged": flagged, "spans": spans, "doc_bytes": doc_bytes, "stats": stats}


def doc_repeats_definition(t, off, arr, lcp, k, mode, scope):
    """the run rule, vectorised: the maximal slot runs with LCP >= k, non-members transparent, mn / mx over the members by
    reduceat; a member p is flagged iff  ANY: mn < p (ALL: or mx > p);  OTHER: mn < ds(p) (ALL: or mx >= de(p))"""
    n = t.size
    offa = np.asarray(off, dtype=np.int64)
    if n == 0:
        return answer_of([], off, 0, k, 0)
    s = np.asarray(arr[1:], dtype=np.int64)                           # slots 1 .. n
    d = np.searchsorted(offa, s, "right") - 1
    ds, de = offa[d], offa[d + 1]
    member = s + k <= de
    head = np.asarray(lcp[1:n + 1], dtype=np.int64) < k               # slot i starts a run (LCP[1] = 0: always)
    first = np.nonzero(head)[0]
    run = np.cumsum(head) - 1
    mn = np.minimum.reduceat(np.where(member, s, 1 << 40), first)[run]
    mx = np.maximum.reduceat(np.where(member, s, -1), first)[run]
    if scope == ANY:
        f = (mn < s) | ((mx > s) if mode == ALL else False)
    else:
        f = (mn < ds) | ((mx >= de) if mode == ALL else False)
    return answer_of(np.sort(s[f & member]), off, n, k, np.count_nonzero(member))


def run_loop_definition(tb, off, arr, lcp, k):
    """the same rule as a plain loop over the runs, all four (mode, scope) pairs in one walk -> {(mode, scope): flagged}"""
    n = len(tb)
    offl = [int(x) for x in off]
    d_of = (np.searchsorted(np.asarray(offl, dtype=np.int64), np.arange(n), "right") - 1).tolist() if n else []
    out = {c: [] for c in COMBOS}
    i = 1
    while i <= n:
        j = i
        while j + 1 <= n and lcp[j + 1] >= k:
            j += 1
        mem = []
        for slot in range(i, j + 1):
            p = int(arr[slot])
            if p + k <= offl[d_of[p] + 1]:
                mem.append((p, offl[d_of[p]], offl[d_of[p] + 1]))
        if mem:
            mn, mx = min(m[0] for m in mem), max(m[0] for m in mem)
            for p, ds, de in mem:
                if mn < p or mx > p:
                    out[(ALL, ANY)].append(p)
                if mn < ds or mx >= de:
                    out[(ALL, OTHER)].append(p)
                if mn < p:
                    out[(KEEP_FIRST, ANY)].append(p)
                if mn < ds:
                    out[(KEEP_FIRST, OTHER)].append(p)
        i = j + 1
    return {c: sorted(v) for c, v in out.items()}


def brute_definition(tb, off, k):
    """the header's words, literally: for every member p, every other member q with the same window decides -- no suffix array,
    no runs -> ({(mode, scope): flagged}, members)"""
    n = len(tb)
    t = _u8(tb)
    offa = np.asarray(off, dtype=np.int64)
    out = {c: [] for c in COMBOS}
    if n == 0:
        return out, 0
    pos = np.arange(n)
    d = np.searchsorted(offa, pos, "right") - 1
    member = pos + k <= offa[d + 1]
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([t, np.zeros(k, dtype=np.uint8)]), k)[:n]
    for p in range(n):
        if not member[p]:
            continue
        q = np.nonzero(member & (pos != p) & np.all(win == win[p], axis=1))[0]
        for qq in q.tolist():                                         # (the double loop: every partner is looked at on its own)
            other = d[qq] != d[p]
            before = qq < p
            if out[(ALL, ANY)][-1:] != [p]:
                out[(ALL, ANY)].append(p)
            if other and out[(ALL, OTHER)][-1:] != [p]:
                out[(ALL, OTHER)].append(p)
            if before and out[(KEEP_FIRST, ANY)][-1:] != [p]:
                out[(KEEP_FIRST, ANY)].append(p)
            if before and other and out[(KEEP_FIRST, OTHER)][-1:] != [p]:
                out[(KEEP_FIRST, OTHER)].append(p)
    return out, int(np.count_nonzero(member))


def ks_of(off, n):
    """1, 2, 3, the shortest non-empty document, one more than the longest document (no members)"""
    lens = np.diff(np.asarray(off, dtype=np.int64))
    ks = {1, 2, 3, int(lens.max()) + 1}
    if np.any(lens > 0):
        ks.add(int(lens[lens > 0].min()))
    return sorted(ks)


def check_text(tb, oracle, rng, tables=None):
    """every table shape (or `tables`) and every k over one text; returns the number of flagged positions seen"""
    t = _u8(tb)
    n = t.size
    arr = oracle.sais(t)
    lcp = _kasai(oracle, t, arr)
    lr = repeat_lengths_definition(t, arr, lcp)
    seen = 0
    all_tables = tables or offset_tables(n, rng)
    loop_tables = set(all_tables) if n <= BRUTE_LIMIT or tables else {"one", "random3", "empty_runs", "more_docs_than_bytes"}
    for name, off in all_tables.items():
        ndocs = len(off) - 1
        if ndocs < 1:
            continue                                                  # (one document per byte of an empty text: no collection)
        for k in ks_of(off, n):
            got = {c: doc_repeats_definition(t, off, arr, lcp, k, *c) for c in COMBOS}
            for c in COMBOS:
                a = got[c]
                assert a["doc_bytes"].size == ndocs and a["spans"].shape[0] <= (n + 1) // (k + 1), (name, k, c)
                assert np.all(a["spans"][:, 1] - a["spans"][:, 0] >= k) and np.all(a["spans"][1:, 0] > a["spans"][:-1, 1])
                seen += a["flagged"].size
            # KEEP_FIRST inside ALL, OTHER inside ANY
            assert np.all(np.isin(got[(KEEP_FIRST, ANY)]["flagged"], got[(ALL, ANY)]["flagged"]))
            assert np.all(np.isin(got[(ALL, OTHER)]["flagged"], got[(ALL, ANY)]["flagged"]))
            assert np.all(np.isin(got[(KEEP_FIRST, OTHER)]["flagged"], got[(KEEP_FIRST, ANY)]["flagged"]))
            if k == int(np.diff(np.asarray(off, dtype=np.int64)).max()) + 1:
                assert all(got[c]["stats"]["members"] == 0 and got[c]["spans"].size == 0 for c in COMBOS), (name, k)
            if name in loop_tables:
                loop = run_loop_definition(tb, off, arr, lcp, k)
                for c in COMBOS:
                    assert got[c]["flagged"].tolist() == loop[c], (name, k, c)
            if n <= BRUTE_LIMIT:
                brute, members = brute_definition(tb, off, k)
                for c in COMBOS:
                    assert got[c]["flagged"].tolist() == brute[c], (name, k, c)
                    assert got[c]["stats"]["members"] == members
            if ndocs == 1:                                            # the identities of the header
                kf_spans, kf_flagged = keep_first_definition(t, arr, lcp, k)
                all_spans, all_flagged = spans_definition(lr, k)
                assert np.array_equal(got[(KEEP_FIRST, ANY)]["spans"], kf_spans)
                assert np.array_equal(got[(KEEP_FIRST, ANY)]["flagged"], kf_flagged)
                assert np.array_equal(got[(ALL, ANY)]["spans"], all_spans)
                assert np.array_equal(got[(ALL, ANY)]["flagged"], all_flagged)
                assert got[(ALL, OTHER)]["flagged"].size == 0 and got[(KEEP_FIRST, OTHER)]["flagged"].size == 0
    return seen


# ---------------------------------------------------------------- tests of the definitions ----

def test_the_header_examples(oracle):
    t = _u8(EXAMPLE_TEXT)
    arr = oracle.sais(t)
    lcp = _kasai(oracle, t, arr)
    a = doc_repeats_definition(t, EXAMPLE_OFF, arr, lcp, 1, KEEP_FIRST, ANY)
    assert a["flagged"].tolist() == [3, 5, 7, 8, 9, 10] and a["spans"].tolist() == [[3, 4], [5, 6], [7, 11]]
    a = doc_repeats_definition(t, EXAMPLE_OFF, arr, lcp, 1, KEEP_FIRST, OTHER)
    assert a["flagged"].tolist() == [5, 7, 8, 9, 10] and a["doc_bytes"].tolist() == [0, 0, 1, 4]
    assert a["stats"] == {"members": 11, "flagged": 5, "spans": 2, "covered_bytes": 5, "docs_touched": 2}
    for scope in (ANY, OTHER):
        assert doc_repeats_definition(t, EXAMPLE_OFF, arr, lcp, 3, ALL, scope)["flagged"].tolist() == [0, 1, 7, 8]
    t = _u8(b"aaaa")
    arr = oracle.sais(t)
    lcp = _kasai(oracle, t, arr)
    for scope in (ANY, OTHER):
        a = doc_repeats_definition(t, [0, 2, 4], arr, lcp, 2, KEEP_FIRST, scope)
        assert a["spans"].tolist() == [[2, 4]] and a["stats"]["members"] == 2
        a = doc_repeats_definition(t, [0, 2, 4], arr, lcp, 2, ALL, scope)
        assert a["spans"].tolist() == [[0, 4]] and a["doc_bytes"].tolist() == [2, 2]
    assert keep_first_definition(t, arr, lcp, 2)[0].tolist() == [[1, 4]]      # the boundary-blind answer
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    assert "KEEP_FIRST, ANY, k = 1 flags {3, 5, 7, 8, 9, 10}: spans {[3,4), [5,6), [7,11)}" in header
    assert "doc_bytes = {0, 0, 1, 4}" in header and "ALL, k = 3, either scope, flags {0, 1, 7, 8}" in header
    assert "sa_amd_repeat_spans gives {[1, 4)}" in header and "{[0, 4)}, merged across the boundary, doc_bytes = {2, 2}" in header
    assert check_text(EXAMPLE_TEXT, oracle, np.random.default_rng(1), {"example": EXAMPLE_OFF}) > 0
    assert check_text(b"aaaa", oracle, np.random.default_rng(1), {"example": [0, 2, 4]}) > 0


def test_definitions_against_the_double_loop_random(oracle):
    rng = np.random.default_rng(17)
    seen = 0
    for trial in range(40):
        n = int(rng.integers(0, 41))
        sigma = int(rng.choice([1, 2, 2, 3, 26]))
        seen += check_text(rng.integers(97, 97 + sigma, n).astype(np.uint8).tobytes(), oracle, rng)
    assert seen > 1000


def test_definitions_on_golden_texts(oracle):
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        manifest = json.load(f)
    rng = np.random.default_rng(18)
    for name in sorted(manifest):
        with open(os.path.join(ROOT, "tests", "golden", name + ".text"), "rb") as f:
            tb = f.read()
        assert len(tb) == manifest[name]["n"]
        check_text(tb, oracle, rng)
    assert len(manifest) >= 5


@pytest.mark.parametrize("name", sorted(adversarial_cases()))
def test_definitions_on_adversarial_cases(oracle, name):
    """every adversarial case of conftest under every table shape: the double loop up to BRUTE_LIMIT bytes, the loop over the runs
    and the ndocs = 1 identities on all of them"""
    tb = adversarial_cases()[name]
    check_text(tb, oracle, np.random.default_rng(len(tb)))


# ---------------------------------------------------------------- header, exports, Python surface ----

def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "suffix_array_amd.h")) as f:
        header = f.read()
    L = ctypes.CDLL(sa.library_path())
    for fn in EXPORTS:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert hasattr(L, fn), fn
    assert re.search(r"#define\s+SA_AMD_DOCREP_ANY\s+0\b", header) and re.search(r"#define\s+SA_AMD_DOCREP_OTHER\s+1\b", header)
    assert (sa.DOCREP_ANY, sa.DOCREP_OTHER) == (ANY, OTHER)
    body = header[header.index("typedef struct sa_amd_doc_repeat_stats"):]
    for field in ("members", "flagged", "spans", "covered_bytes", "docs_touched", "readbacks", "reserved"):
        assert field in dict(sa.DocRepeatStats._fields_), field
        assert re.search(r"\b" + field + r"\b", body), field
    assert ctypes.sizeof(sa.DocRepeatStats) == 5 * 8 + 2 * 4
    with open(os.path.join(ROOT, "suffix_array_amd", "csrc", "kernels", "doc_repeats.hpp")) as f:
        kernels = f.read()
    assert re.search(r"constexpr int DOCREP_ANY = 0, DOCREP_OTHER = 1;", kernels)
    with open(os.path.join(ROOT, "include", "suffix_array_amd.hpp")) as f:
        assert re.search(r"\brepeat_spans\s*\(std::int32_t min_len, std::int32_t mode", f.read())


def test_python_surface():
    def params(fn):
        return list(inspect.signature(fn).parameters)
    for cls in (sa.DeviceIndex, sa.SuffixArray):
        sig = inspect.signature(cls.doc_repeat_spans)
        assert list(sig.parameters) == ["self", "min_len", "mode", "scope", "doc_bytes"]
        assert sig.parameters["mode"].default == sa.REPEATS_KEEP_FIRST and sig.parameters["scope"].default == sa.DOCREP_OTHER
        assert sig.parameters["doc_bytes"].default is False
    assert params(sa.doc_repeats_work_bytes) == ["n", "ndocs"] and params(sa.last_doc_repeat_stats) == []
    for name in ("DocRepeatStats", "last_doc_repeat_stats", "doc_repeats_work_bytes", "DOCREP_ANY", "DOCREP_OTHER"):
        assert name in sa.__all__ and hasattr(sa, name), name


def test_argument_checks_answer_without_a_device():
    L = sa.lib()
    buf = np.full(64, 0x77777777, dtype=np.uint32)
    p = buf.ctypes.data
    cnt = ctypes.c_int64(-5)
    c = ctypes.byref(cnt)
    assert L.sa_amd_doc_repeats_work_bytes(-1, 1) == -1 and L.sa_amd_doc_repeats_work_bytes(4, 0) == -1
    assert L.sa_amd_doc_repeats_work_bytes(4, -2) == -1
    for mode in (ALL, KEEP_FIRST):
        for scope in (ANY, OTHER):
            assert L.sa_amd_index_doc_repeat_spans(None, 2, mode, scope, p, 4, c, p + 128) == -1          # NULL index
    assert cnt.value == -5 and np.all(buf == 0x77777777)
    L.sa_amd_last_doc_repeat_stats(None)
    st = sa.last_doc_repeat_stats()
    assert set(st) == {"members", "flagged", "spans", "covered_bytes", "docs_touched", "readbacks"}


@pytest.mark.parametrize("n,ndocs", [(0, 1), (1, 1), (4095, 9000), (1 << 20, 256), (2**31 - 1, 1 << 16)])
def test_work_block(n, ndocs):
    """the repeat finder's block plus one word per document"""
    w = sa.doc_repeats_work_bytes(n, ndocs)
    r = sa.repeats_work_bytes(n)
    assert w % 256 == 0 and r + 4 * ndocs <= w <= r + 4 * ndocs + 512
