"""A C++ caller of suffix_array::DocumentIndex::infgram_score (include/suffix_array_amd.hpp): the example of the header's section
on scoring a text under the infinity-gram model, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index(tmp_path):
    src = tmp_path / "score_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::uint8_t> U8;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    const std::size_t n = std::strlen(txt);
    DocumentIndex ix(t, n, U32{0, 11});                               // the array is built on the device
    auto r = ix.infgram_score("xcabra", 1, 4);
    if (r.size() != 6) return 1;
    if (r.s != U32{0, 0, 1, 2, 2, 3} || r.lo != U32{0, 0, 8, 8, 2, 2} || r.hi != U32{12, 12, 9, 9, 4, 4}) return 2;
    if (r.at_end != U8{1, 1, 0, 0, 0, 0} || r.nlo != U32{12, 8, 8, 8, 2, 2} || r.nhi != U32{12, 9, 9, 8, 4, 4}) return 3;
    if (r.count(1) != 1 || r.total(1) != 11 || r.count(0) != 0 || r.count(4) != 2 || r.total(4) != 2) return 4;
    r = ix.infgram_score("xcabra", 3, 4);
    if (r.s[5] != 0 || r.lo[5] != 0 || r.hi[5] != 12 || r.count(5) != 5) return 5;       // the unigram count of 'a'
    r = ix.infgram_score("xcabra", 1, 4, {0, 0, 4, 6});                // documents "", "xcab", "ra": a context stops at its start
    if (r.s != U32{0, 0, 1, 2, 0, 1} || r.lo[5] != 10 || r.hi[5] != 12 || r.at_end[5] != 0 || r.nlo[5] != 10 || r.nhi[5] != 12) return 6;
    r = ix.infgram_score("xcabra");                                   // the default cap
    if (r.s != U32{0, 0, 1, 2, 2, 3}) return 7;
    if (ix.infgram_score("").size() != 0 || ix.infgram_score("", 1, 4, {0, 0}).size() != 0) return 8;
    try { ix.infgram_score("a", 0); return 9; } catch (const std::invalid_argument &) { }
    try { ix.infgram_score("a", 1, 0); return 10; } catch (const std::invalid_argument &) { }
    try { ix.infgram_score("a", 1, SA_AMD_SCORE_MAX_CONTEXT + 1); return 11; } catch (const std::invalid_argument &) { }
    try { ix.infgram_score("abc", 1, 4, {0, 2}); return 12; } catch (const std::exception &) { }       // offsets that do not end at m
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "score_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
