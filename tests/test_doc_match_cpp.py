"""A C++ caller of suffix_array::DocumentIndex::match / match_list (include/suffix_array_amd.hpp): the example of
include/suffix_array_amd_docmatch.h, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index_match(tmp_path):
    src = tmp_path / "doc_match_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::Clause;
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<Clause> Query;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    DocumentIndex ix(t, std::strlen(txt), U32{0, 4, 4, 7, 11});      // "abra", "", "cad", "abra"
    const std::vector<Query> queries = {
        { {{"a"}, false}, {{"bra"}, false} },                         // a AND bra
        { {{"a"}, false}, {{"bra"}, true} },                          // a AND NOT bra
        { {{"a"}, true} },                                            // NOT a
        { {{"c", "bra"}, false} },                                    // (c OR bra)
        { {{"ac"}, false} },                                          // across the boundary at byte 3: document 0
        { {{"a"}, false}, {{"c"}, false}, {{"bra"}, false} },
        { },                                                          // no clauses: every document
    };
    if (ix.match(queries) != U32{2, 1, 1, 3, 1, 0, 4}) return 1;
    const auto ls = ix.match_list(queries);
    if (ls.size() != 7 || ls[0] != U32{0, 3} || ls[1] != U32{2} || ls[2] != U32{1} || ls[3] != U32{0, 2, 3} || ls[4] != U32{0}) return 2;
    if (!ls[5].empty() || ls[6] != U32{0, 1, 2, 3}) return 3;
    if (!ix.match({}).empty() || !ix.match_list({}).empty()) return 4;
    Clause none;                                                      // a clause without patterns holds nowhere; negated, everywhere
    Clause all;
    all.negate = true;
    if (ix.match({ Query{none}, Query{all}, Query{all, Clause{{"cad"}, false}} }) != U32{0, 4, 1}) return 5;
    sa_amd_doc_match_stats st;
    sa_amd_last_doc_match_stats(&st);
    if (st.queries != 3 || st.clauses != 4 || st.patterns != 1 || st.marks != 1 || st.bitmap_words != 1 || st.slabs != 1 || st.listed != 0) return 6;
    ix.set_documents(U32{0, 11});                                     // replaced: one document
    if (ix.match({ Query{Clause{{"a"}, false}, Clause{{"zz"}, true}} }) != U32{1} || ix.match_list({ Query{Clause{{"zz"}, false}} })[0] != U32{}) return 7;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "doc_match_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
