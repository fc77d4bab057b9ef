"""GPU test of the device index as the owner of its tables (csrc/host/index.hpp): every route that installs or replaces a table --
buckets, enable_lcp, set_documents, enable_doc_freq, set_documents again, enable_doc_freq again -- with one search, one
doc_search and one doc_topk after each step against the models of tests/test_lcp_search_abi.py, tests/test_docs_abi.py and
tests/test_doc_tf_abi.py; then both shapes of destroy (every table built, no table at all).  Twice in one process.

Sizes: a 4 KiB text of tests/golden (the smallest at which every table exists and the collection's sort runs) and the empty text
with one empty document."""
import os

import numpy as np
import pytest

import suffix_array_amd as sa
import search_model
from test_docs_abi import answers_definition as docs_answers
from test_doc_tf_abi import answers_definition as tf_answers, topk_definition
from test_lcp_search_abi import esa_search, kasai, pair_table

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 3
_MODELS = {}


def _text(name):
    """-> (text, bytes, suffix array, pair table, bucket table) of a golden fixture, or of the empty text; computed once"""
    if name not in _MODELS:
        tb = b""
        arr = np.zeros(1, dtype=np.uint32)
        if name:
            with open(os.path.join(GOLDEN, name + ".text"), "rb") as f:
                tb = f.read()
            arr = np.fromfile(os.path.join(GOLDEN, name + ".sa.u32le"), dtype="<u4").astype(np.uint32)
        t = np.frombuffer(tb, dtype=np.uint8) if tb else np.zeros(0, dtype=np.uint8)
        _MODELS[name] = (t, tb, arr, pair_table(kasai(tb, arr)), np.asarray(search_model.bucket_table(tb), dtype=np.uint32))
    return _MODELS[name]


def _patterns(tb):
    n = len(tb)
    cut = [tb[a:a + k] for a, k in ((0, 1), (n // 3, 2), (n // 2, 5), (n // 5, 40), (max(n - 3, 0), 3))] if n else []
    return [b"", b"e", b"th", b"\x01\x02nope", b"\xff"] + [p for p in cut if p] + ([tb[7:19] + b"\x00"] if n else [])


def _check(ix, name, pats, bkt, off, freq):
    """one search, one doc_search and one doc_topk of `ix`, which has the bucket table iff `bkt`, the collection `off` (or none)
    and the frequency table iff `freq`"""
    t, tb, arr, pair, _ = _text(name)
    got = ix.search(pats)
    for q, pat in enumerate(pats):
        exp, _ = esa_search(tb, arr, pair, pat, bkt)
        assert (bool(got["contains"][q]), int(got["lo"][q]), int(got["hi"][q]), int(got["lcp_start"][q]), int(got["lcp_len"][q])) == exp, pat[:16]
    if off is None:
        with pytest.raises(sa.SuffixArrayError):
            ix.doc_search(pats)
    else:
        occ, df, _ = docs_answers(tb, off, arr, pats)
        got_occ, got_df = ix.doc_search(pats)
        assert np.array_equal(got_occ, occ) and np.array_equal(got_df, df)
    if not freq:
        with pytest.raises(sa.SuffixArrayError):                      # no collection, or its frequency table is not (or no longer) there
            ix.doc_topk(pats, K)
    else:
        top = ix.doc_topk(pats, K)
        for q, (_, ls, tf) in enumerate(tf_answers(tb, off, arr, pats)):
            docs, freqs = topk_definition(ls, tf, K)
            assert np.array_equal(top[q][0], docs) and np.array_equal(top[q][1], freqs), pats[q][:16]


def _walk(name, first, second):
    t, tb, arr, _, table = _text(name)
    pats = _patterns(tb)
    ix = sa.DeviceIndex(t, arr)
    _check(ix, name, pats, None, None, False)
    assert np.array_equal(ix.buckets(), table)
    _check(ix, name, pats, table, None, False)
    assert np.array_equal(ix.buckets(), table)                        # the kept table, not a second build
    ix.enable_lcp()
    _check(ix, name, pats, table, None, False)
    assert sa.last_search_stats()["route"] == 1
    ix.set_documents(first)
    _check(ix, name, pats, table, first, False)
    ix.enable_doc_freq()
    _check(ix, name, pats, table, first, True)
    with pytest.raises(sa.SuffixArrayError):                          # a refused collection: the old one and its frequency table stay
        ix.set_documents([0, len(tb) + 1])
    _check(ix, name, pats, table, first, True)
    ix.set_documents(second)                                          # the frequency table was the old collection's
    _check(ix, name, pats, table, second, False)
    ix.enable_doc_freq()
    ix.enable_doc_freq()                                              # a no-op the second time
    _check(ix, name, pats, table, second, True)
    assert np.array_equal(ix.suffix_array(), arr) and (not len(tb) or ix.check_integrity())
    ix.close()                                                        # every table built
    ix = sa.DeviceIndex(t)                                            # the array built on the device; no table at all
    assert np.array_equal(ix.suffix_array(), arr)
    ix.close()


def test_every_install_and_replace_path_then_both_destroy_shapes():
    n = 4096
    assert _text("english_4k_seed3")[0].size == n
    rng = np.random.default_rng(31)
    first = np.concatenate([[0], np.sort(rng.integers(0, n + 1, 11)), [n]])
    second = np.concatenate([[0, 0], np.sort(rng.integers(0, n + 1, 300)), [n, n]])      # (more documents, empty ones at both ends)
    for _ in range(2):                                                # (twice in one process: what the first walk freed is gone for good)
        _walk("english_4k_seed3", first, second)
        _walk("", [0, 0], [0, 0, 0])                                  # n = 0: one empty document, then two
