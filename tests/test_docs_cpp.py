"""A C++ caller of suffix_array::DocumentIndex (include/suffix_array_amd.hpp): the example of the header's section on document
collections, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index(tmp_path):
    src = tmp_path / "docs_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    const std::size_t n = std::strlen(txt);
    DocumentIndex ix(t, n, U32{0, 4, 4, 7, 11});                     // "abra", "", "cad", "abra"; the array is built on the device
    const auto sd = ix.doc_search({"a", "bra", "", "zz"});
    if (sd.size() != 4) return 1;
    if (sd[0] != std::make_pair(5u, 3u) || sd[1] != std::make_pair(2u, 2u) || sd[2] != std::make_pair(12u, 3u) || sd[3] != std::make_pair(0u, 0u)) return 2;
    const auto ls = ix.doc_list({"a", "bra", "zz", "cad"});
    if (ls.size() != 4 || ls[0] != U32{3, 0, 2} || ls[1] != U32{3, 0} || !ls[2].empty() || ls[3] != U32{2}) return 3;
    if (ix.doc_of(U32{0, 3, 4, 6, 7, 10, 11, 0xffffffffu}) != U32{0, 0, 2, 2, 3, 3, SA_AMD_DOC_NONE, SA_AMD_DOC_NONE}) return 4;
    try { ix.set_documents(U32{0, 5, 4, 11}); return 5; } catch (const std::invalid_argument &) { }     // malformed: the old one stays
    try { ix.set_documents(U32{0}); return 6; } catch (const std::invalid_argument &) { }
    if (ix.doc_list({"a"})[0] != U32{3, 0, 2}) return 7;
    ix.set_documents(U32{0, 11});                                     // replaced: one document
    if (ix.doc_search({"a"})[0] != std::make_pair(5u, 1u) || ix.doc_list({"bra"})[0] != U32{0}) return 8;
    const std::uint32_t want[12] = { 11, 10, 7, 0, 3, 5, 8, 1, 4, 6, 9, 2 };
    DocumentIndex own(t, n, U32{0, 4, 4, 7, 11}, want);              // the caller's array
    if (own.doc_list({"a"})[0] != U32{3, 0, 2}) return 9;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "docs_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
