"""The two guards of DESIGN.md section 10 on the document calls of the token indexes (include/sa_amd_tokdocs.h), through the
diagnostic library: no answer depends on the bytes a pooled block or a table held before the call (every fill pattern of
tests/dirty_blocks.py), and a refused memory request is SA_AMD_ENOMEM with nothing written, the previous collection still
answering and nothing leaked -- or the documented read-back by copy with the same answers.

The pinned suites (tests/test_dirty_blocks.py, tests/test_refused_allocs.py) read their calls from the main header and the
sub-headers it names; these sixteen are declared in a header of their own, so their prototypes are declared here and the cases
follow the same numbered properties: one count-only pass per call names its requests, then one case per request."""
import ctypes
import functools

import numpy as np
import pytest

import suffix_array_amd as sa
import dirty_blocks
import refused_allocs as ra
from refused_allocs import ENOMEM, OK, out
from test_gpu_parity import _hip
from test_token_docs import CLS, WIDTHS, collections, defined_answers, device_answers, first_difference, patterns_for, widen, widen_queries
from test_token_docs_abi import OPS, PREFIXES, queries_of, separator_offsets
from test_tokens_abi import brute_suffix_array, families

pytestmark = pytest.mark.gpu

N = 600
D, P, Tb = "device", "pinned", "table"
READBACK = "read-back by copy: read_words remembers the refused pinned block for the thread and copies instead (host/readback.hpp)"
VP, I32, I64, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
PROTOTYPES = {                          # the declarations of include/sa_amd_tokdocs.h (tests/test_token_docs_abi.py pins the wrapper's copies)
    "set_documents": [VP, VP, I64], "set_documents_by_separator": [VP, U32, VP], "doc_offsets": [VP, VP, I64, VP], "doc_of": [VP, VP, I64, VP],
    "doc_search": [VP, VP, VP, I32, VP, VP], "doc_list": [VP, VP, VP, I32, VP, VP, I64, VP],
    "doc_match": [VP, VP, VP, I32, VP, VP, I32, VP, I32, VP, VP], "doc_match_list": [VP, VP, VP, I32, VP, VP, I32, VP, I32, VP, VP, I64, VP],
}
assert tuple(PROTOTYPES) == OPS
# op -> (the requests of one successful call in order, k -> why request k refused is no error)
REQUESTS = {
    "set_documents": ((Tb, Tb, D, P), {4: READBACK}),
    "set_documents_by_separator": ((D, P, Tb, Tb), {2: READBACK}),
    "doc_offsets": ((), {}),
    "doc_of": ((D,), {}),
    "doc_search": ((D, P), {2: READBACK}),
    "doc_list": ((D, P, D), {2: READBACK}),
    "doc_match": ((D, P, D), {2: READBACK}),
    "doc_match_list": ((D, P, D), {2: READBACK}),
}


@functools.lru_cache(maxsize=None)
def case():
    """the text, its array, two collections, the patterns and queries, and what the definitions answer under each collection"""
    t = [int(x) for x in families(N)["zipf_50000"]]
    arr = brute_suffix_array(t).tolist()
    rng = np.random.default_rng(23)
    first = collections(N, rng)["random_cuts"]
    sep = t[7]
    second = separator_offsets(np.array(t), sep).tolist()
    assert 2 < len(second) and second != first
    pats = patterns_for(t, first, rng)[:14]
    queries = queries_of(pats, rng)
    pos = np.arange(0, N + 3, 3, dtype=np.uint32)
    want = {name: defined_answers(t, arr, off, pats, queries, pos) for name, off in (("first", first), ("second", second))}
    return {"t": t, "first": first, "second": second, "sep": sep, "pats": pats, "queries": queries, "pos": pos, "want": want}


# ---------------------------------------------------------------- dirty blocks ----

@pytest.mark.parametrize("pattern", dirty_blocks.ORDER)
@pytest.mark.parametrize("width", WIDTHS)
def test_every_call_on_blocks_that_hold_arbitrary_bytes(width, pattern):
    c = case()
    with dirty_blocks.diag_library() as d:
        d.fill(pattern)
        ix = d._track(CLS[width](widen(c["t"], width)))
        for chunk, budget in ((64, 4096), (-1, -1)):
            prev = sa.docs_set_chunk(chunk), sa.doc_match_set_budget(budget)
            try:
                assert ix.set_documents(c["first"]) == len(c["first"]) - 1
                got = device_answers(ix, width, c["pats"], c["queries"], c["pos"])
                assert first_difference(got, c["want"]["first"]) is None, (pattern, chunk, first_difference(got, c["want"]["first"]))
                assert ix.set_documents(separator=int(widen([c["sep"]], width)[0])) == len(c["second"]) - 1
                got = device_answers(ix, width, c["pats"], c["queries"], c["pos"])
                assert first_difference(got, c["want"]["second"]) is None, (pattern, chunk, first_difference(got, c["want"]["second"]))
            finally:
                sa.docs_set_chunk(prev[0])
                sa.doc_match_set_budget(prev[1])


# ---------------------------------------------------------------- refused allocations ----

def _listing(lists):
    return (np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64),
            np.array([d for l in lists for d in l], dtype=np.uint32))


def call_args(op, width, ix):
    """name -> value in the declaration's order; the outputs are fresh arrays"""
    c = case()
    data, off, cnt = ix._batch([widen(p, width) for p in c["pats"]])
    qd, qoff, npat, coff, cfl, ncl, qo, nq = ix._queries(widen_queries(c["queries"], width))
    w = c["want"]["first"]
    lead = dict(ix=ix, pat_data=data, pat_off=off, count=cnt)
    qlead = dict(ix=ix, pat_data=qd, pat_off=qoff, npat=npat, clause_off=coff, clause_flags=cfl, nclauses=ncl, query_off=qo, nqueries=nq)
    if op == "set_documents":
        return dict(ix=ix, doc_off=np.array(c["second"], dtype=np.uint32), ndocs=len(c["second"]) - 1)
    if op == "set_documents_by_separator":
        return dict(ix=ix, separator=int(widen([c["sep"]], width)[0]), ndocs_out=out(1, np.int64))
    if op == "doc_offsets":
        return dict(ix=ix, doc_off_out=out(len(c["first"]) + 3), capacity=len(c["first"]) + 3, ndocs_out=out(1, np.int64))
    if op == "doc_of":
        return dict(ix=ix, pos=c["pos"], count=c["pos"].size, doc_out=out(c["pos"].size))
    if op == "doc_search":
        return dict(lead, occ=out(cnt), df=out(cnt))
    if op == "doc_list":
        total = sum(w["df"])
        return dict(lead, list_off=out(cnt + 1, np.int64), docs=out(total + 5), capacity=total + 5, total_out=out(1, np.int64))
    if op == "doc_match":
        return dict(qlead, df=out(nq), clause_df=out(ncl))
    total = sum(w["mdf"])
    return dict(qlead, list_off=out(nq + 1, np.int64), docs=out(total + 5), capacity=total + 5, total_out=out(1, np.int64))


OUTPUTS = {"set_documents": (), "set_documents_by_separator": ("ndocs_out",), "doc_offsets": ("doc_off_out", "ndocs_out"), "doc_of": ("doc_out",),
           "doc_search": ("occ", "df"), "doc_list": ("list_off", "docs", "total_out"), "doc_match": ("df", "clause_df"),
           "doc_match_list": ("list_off", "docs", "total_out")}


def answers_exact(op, width, ix, a, rc):
    """a successful call's answers are the definitions' (the collection under which it ran: "first"; the two that set one leave "second")"""
    c = case()
    w = c["want"]["first"]
    if rc != OK:
        return False
    if op in ("set_documents", "set_documents_by_separator"):
        ok = op == "set_documents" or int(a["ndocs_out"][0]) == len(c["second"]) - 1
        return ok and first_difference(device_answers(ix, width, c["pats"], c["queries"], c["pos"]), c["want"]["second"]) is None
    if op == "doc_offsets":
        m = len(c["first"])
        return a["doc_off_out"][:m].tolist() == c["first"] and ra.untouched(a["doc_off_out"][m:]) and int(a["ndocs_out"][0]) == m - 1
    if op == "doc_of":
        return a["doc_out"].tolist() == w["doc_of"]
    if op == "doc_search":
        return a["occ"].tolist() == w["occ"] and a["df"].tolist() == w["df"]
    if op == "doc_match":
        return a["df"].tolist() == w["mdf"] and a["clause_df"].tolist() == w["cdf"]
    loff, docs = _listing(w["lists"] if op == "doc_list" else w["mlists"])
    return (np.array_equal(a["list_off"], loff) and np.array_equal(a["docs"][:docs.size], docs) and ra.untouched(a["docs"][docs.size:])
            and int(a["total_out"][0]) == docs.size)


class Harness:
    def __init__(self, d):
        self.d = d
        self.L = ctypes.CDLL(sa.library_path())                       # (the diagnostic library: the wrapper points at it)
        for prefix in PREFIXES.values():
            for op, argtypes in PROTOTYPES.items():
                f = getattr(self.L, prefix + op)
                f.argtypes, f.restype = argtypes, I32
        self.L.sa_amd_release_cache.argtypes, self.L.sa_amd_release_cache.restype = [], None
        self.hooks = ra.Hooks(self)
        self.hip = _hip()
        self.kinds = {}

    def ledger_after_release(self):
        self.L.sa_amd_release_cache()
        return self.hooks.ledger()

    def index(self, width):
        """an index with the first collection, made on the pytest thread: the case's thread starts with no read-back block"""
        ix = self.d._track(CLS[width](widen(case()["t"], width)))
        ix.set_documents(case()["first"])
        return ix

    def one_call(self, op, width, ix, nth):
        a = call_args(op, width, ix)
        outs = {k: a[k] for k in OUTPUTS[op]}
        ra.fill_canary(outs)
        self.hooks.refuse(nth)
        try:
            rc = getattr(self.L, PREFIXES[width] + op)(*[ra.as_argument(v) for v in a.values()])
            fired, kinds = self.hooks.fired(), self.hooks.kinds()
        finally:
            made = self.hooks.refuse(-1)
        return a, outs, rc, fired, made, kinds, int(self.hip.hipPeekAtLastError())

    def count_pass(self, op, width):
        if (op, width) not in self.kinds:
            ix = self.index(width)
            try:
                def work():
                    a, outs, rc, fired, made, kinds, peek = self.one_call(op, width, ix, 0)
                    assert answers_exact(op, width, ix, a, rc), (op, width, "the answers of the count-only pass", rc)
                    assert fired == 0 and peek == 0 and made == len(kinds), (fired, peek, made, kinds)
                    return kinds
                self.kinds[(op, width)] = ra.on_a_fresh_thread(work)
            finally:
                ix.close()
        return self.kinds[(op, width)]

    def refused(self, op, width, k):
        want_kinds, fallbacks = REQUESTS[op]
        assert self.count_pass(op, width) == want_kinds
        before = self.ledger_after_release()
        c = case()
        ix = self.index(width)
        try:
            def work():
                a, outs, rc, fired, made, kinds, peek = self.one_call(op, width, ix, k)
                where = (op, width, k, want_kinds[k - 1], rc)
                assert fired == 1 and made >= k and kinds[:k] == want_kinds[:k], ("1: the refusal fired once, at request k", where, fired, made)
                assert rc == ENOMEM or answers_exact(op, width, ix, a, rc), ("1/3: SA_AMD_ENOMEM, or a success with exact answers", where)
                if rc == ENOMEM:
                    assert k not in fallbacks, ("3: a listed fallback answered SA_AMD_ENOMEM", where)
                    written = [name for name, arr in outs.items() if not ra.untouched(arr)]
                    assert not written, ("2: outputs written by a call that answered SA_AMD_ENOMEM", where, written)
                    got = device_answers(ix, width, c["pats"], c["queries"], c["pos"])
                    assert first_difference(got, c["want"]["first"]) is None, ("2: the previous collection no longer answers", where)
                else:
                    assert k in fallbacks, ("3: a success that is no listed fallback", where)
                assert peek == 0, ("4: the runtime's error is pending on the thread", where, peek)
                if rc == OK and op.startswith("set_documents"):        # the armed call changed the collection: back to the first
                    ix.set_documents(c["first"])
                a2, _, rc2, _, _, _, peek2 = self.one_call(op, width, ix, 0)
                assert answers_exact(op, width, ix, a2, rc2) and peek2 == 0, ("5: the un-armed call that follows", where, rc2, peek2)
            ra.on_a_fresh_thread(work)
        finally:
            ix.close()
        after = self.ledger_after_release()
        assert after == before, ("6: the ledger (device, pinned) after the case", op, width, k, before, after)


@pytest.fixture(scope="module")
def harness():
    with dirty_blocks.diag_library() as d:
        h = Harness(d)
        h.index(16).close()             # (the pytest thread takes its own read-back block now, outside every case's ledger)
        yield h


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("width", WIDTHS)
def test_requests_of_a_call(harness, width, op):
    assert harness.count_pass(op, width) == REQUESTS[op][0], (op, width)


REFUSALS = [pytest.param(w, op, k, id="%d-%s-k%d-%s" % (w, op, k, kinds[k - 1])) for w in WIDTHS for op, (kinds, _) in REQUESTS.items()
            for k in range(1, len(kinds) + 1)]


@pytest.mark.parametrize("width,op,k", REFUSALS)
def test_refused_request(harness, width, op, k):
    harness.refused(op, width, k)
