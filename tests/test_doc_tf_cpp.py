"""A C++ caller of the term-frequency methods of suffix_array::DocumentIndex (include/suffix_array_amd.hpp): the example of the
header's section on term frequencies and top-k documents, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index(tmp_path):
    src = tmp_path / "doc_tf_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::pair<std::uint32_t, std::uint32_t>> Pairs;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    const std::size_t n = std::strlen(txt);
    DocumentIndex ix(t, n, U32{0, 4, 4, 7, 11});                     // "abra", "", "cad", "abra"; the array is built on the device
    try { ix.term_frequencies({"a"}); return 1; } catch (const std::invalid_argument &) { }     // no table yet
    try { ix.top_k({"a"}, 1); return 2; } catch (const std::invalid_argument &) { }
    ix.enable_frequencies();
    ix.enable_frequencies();                                          // a no-op the second time
    const auto tf = ix.term_frequencies({"a", "bra", "", "zz"});
    if (tf.size() != 4 || tf[0] != Pairs{{3, 2}, {0, 2}, {2, 1}} || tf[1] != Pairs{{3, 1}, {0, 1}}) return 3;
    if (tf[2] != Pairs{{3, 4}, {0, 4}, {2, 3}} || !tf[3].empty()) return 4;
    if (ix.top_k({"a"}, 1)[0] != Pairs{{0, 2}}) return 5;
    if (ix.top_k({"a"}, 2)[0] != Pairs{{0, 2}, {3, 2}}) return 6;
    const auto top = ix.top_k({"a", "zz", ""}, 5);
    if (top.size() != 3 || top[0] != Pairs{{0, 2}, {3, 2}, {2, 1}} || !top[1].empty() || top[2] != Pairs{{0, 4}, {3, 4}, {2, 3}}) return 7;
    try { ix.top_k({"a"}, 0); return 8; } catch (const std::invalid_argument &) { }
    try { ix.top_k({"a"}, SA_AMD_DOC_TOPK_MAX + 1); return 9; } catch (const std::invalid_argument &) { }
    if (!ix.term_frequencies({}).empty() || !ix.top_k({}, 3).empty()) return 10;
    ix.set_documents(U32{0, 11});                                     // replaced: the table went with the old collection
    try { ix.top_k({"a"}, 1); return 11; } catch (const std::invalid_argument &) { }
    ix.enable_frequencies();
    if (ix.term_frequencies({"a"})[0] != Pairs{{0, 5}} || ix.top_k({"bra"}, 4)[0] != Pairs{{0, 2}}) return 12;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "doc_tf_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
