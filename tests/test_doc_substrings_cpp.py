"""A C++ caller of suffix_array::DocumentIndex::repeated_substrings (include/suffix_array_amd.hpp): the examples of the header's
section on repeated substrings with their document frequency, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index_repeated_substrings(tmp_path):
    src = tmp_path / "doc_substrings_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<DocumentIndex::DocSubstring> Rows;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    DocumentIndex ix(t, std::strlen(txt), U32{0, 4, 4, 7, 11});      // "abra", "", "cad", "abra"; the array is built on the device
    // (lo, count, depth, parent, pos, df): "a", "abra", "bra", "ra"
    if (ix.repeated_substrings() != Rows{{1, 5, 1, 0, 10, 3}, {2, 2, 4, 1, 7, 2}, {6, 2, 3, 0, 8, 2}, {10, 2, 2, 0, 9, 2}}) return 1;
    if (ix.repeated_substrings(1, 0, 2, 3) != Rows{{1, 5, 1, 0, 10, 3}}) return 2;                                  // min_docs = 3
    if (!ix.repeated_substrings(1, 0, 2, 4).empty()) return 3;
    if (ix.repeated_substrings(1, 0, 2, 1, SA_AMD_SUBSTR_BY_DOCS, 2) != Rows{{1, 5, 1, 0, 10, 3}, {2, 2, 4, 1, 7, 2}}) return 4;
    if (ix.repeated_substrings(1, 0, 2, 2, SA_AMD_SUBSTR_BY_LENGTH, 1) != Rows{{2, 2, 4, 1, 7, 2}}) return 5;       // longest in two documents
    if (ix.repeated_substrings(2, 3, 2, 2, SA_AMD_SUBSTR_BY_COVER, 9) != Rows{{2, 2, 4, 1, 7, 2}, {6, 2, 3, 0, 8, 2}, {10, 2, 2, 0, 9, 2}}) return 6;
    try { ix.repeated_substrings(1, 0, 2, 0); return 7; } catch (const std::invalid_argument &) { }                  // min_docs = 0
    try { ix.repeated_substrings(1, 0, 2, 1, 5, 1); return 8; } catch (const std::invalid_argument &) { }            // order 5
    try { ix.repeated_substrings(1, 0, 2, 1, SA_AMD_SUBSTR_BY_DOCS); return 9; } catch (const std::invalid_argument &) { }      // k = 0
    ix.set_documents(U32{0, 11});                                     // one document: every df is 1
    for (const auto &r : ix.repeated_substrings()) if (r.df != 1) return 10;
    if (ix.repeated_substrings().size() != 4) return 11;
    const char *a4 = "aaaa";
    const std::uint32_t want[5] = { 4, 3, 2, 1, 0 };
    DocumentIndex own(reinterpret_cast<const std::uint8_t *>(a4), 4, U32{0, 2, 4}, want);       // the caller's array
    if (own.repeated_substrings() != Rows{{1, 4, 1, 0, 3, 2}, {2, 3, 2, 1, 2, 2}, {3, 2, 3, 2, 1, 1}}) return 12;
    sa_amd_doc_substr_stats st;
    sa_amd_last_doc_substr_stats(&st);
    if (st.nodes != 3 || st.selected != 3 || st.df_sum != 5 || st.max_df != 2 || st.pairs != 2) return 13;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "doc_substrings_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
