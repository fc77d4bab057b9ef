"""A C++ caller of suffix_array::DocumentIndex::repeat_spans (include/suffix_array_amd.hpp): the examples of the header's section
on document-aware duplicate spans, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index_repeat_spans(tmp_path):
    src = tmp_path / "doc_repeats_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::pair<std::uint32_t, std::uint32_t>> Spans;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    DocumentIndex ix(t, std::strlen(txt), U32{0, 4, 4, 7, 11});      // "abra", "", "cad", "abra"; the array is built on the device
    if (ix.repeat_spans(1, SA_AMD_REPEATS_KEEP_FIRST, SA_AMD_DOCREP_ANY) != Spans{{3, 4}, {5, 6}, {7, 11}}) return 1;
    U32 db;
    if (ix.repeat_spans(1, SA_AMD_REPEATS_KEEP_FIRST, SA_AMD_DOCREP_OTHER, &db) != Spans{{5, 6}, {7, 11}}) return 2;
    if (db != U32{0, 0, 1, 4}) return 3;
    if (ix.repeat_spans(1) != Spans{{5, 6}, {7, 11}}) return 4;       // the defaults: KEEP_FIRST, OTHER
    if (ix.repeat_spans(3, SA_AMD_REPEATS_ALL, SA_AMD_DOCREP_ANY) != Spans{{0, 4}, {7, 11}}) return 5;
    if (ix.repeat_spans(3, SA_AMD_REPEATS_ALL, SA_AMD_DOCREP_OTHER, &db) != Spans{{0, 4}, {7, 11}} || db != U32{4, 0, 0, 4}) return 6;
    if (!ix.repeat_spans(5, SA_AMD_REPEATS_ALL, SA_AMD_DOCREP_ANY, &db).empty() || db != U32{0, 0, 0, 0}) return 7;      // no members
    try { ix.repeat_spans(0); return 8; } catch (const std::invalid_argument &) { }
    try { ix.repeat_spans(2, 7, SA_AMD_DOCREP_ANY); return 9; } catch (const std::invalid_argument &) { }
    try { ix.repeat_spans(2, SA_AMD_REPEATS_ALL, 2); return 10; } catch (const std::invalid_argument &) { }
    ix.set_documents(U32{0, 11});                                     // one document: OTHER has nothing, ANY is the boundary-blind answer
    if (!ix.repeat_spans(1).empty()) return 11;
    if (ix.repeat_spans(4, SA_AMD_REPEATS_KEEP_FIRST, SA_AMD_DOCREP_ANY, &db) != Spans{{7, 11}} || db != U32{4}) return 12;
    const char *a4 = "aaaa";
    const std::uint32_t want[5] = { 4, 3, 2, 1, 0 };
    DocumentIndex own(reinterpret_cast<const std::uint8_t *>(a4), 4, U32{0, 2, 4}, want);       // the caller's array
    if (own.repeat_spans(2) != Spans{{2, 4}}) return 13;
    if (own.repeat_spans(2, SA_AMD_REPEATS_ALL, SA_AMD_DOCREP_OTHER, &db) != Spans{{0, 4}} || db != U32{2, 2}) return 14;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "doc_repeats_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
