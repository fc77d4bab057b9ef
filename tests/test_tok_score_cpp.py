"""A C++ caller of suffix_array::TokenIndex::infgram_score (include/suffix_array_amd.hpp): the example of the header's section on
scoring a token text under the infinity-gram model, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_token_index_infgram_score(tmp_path):
    src = tmp_path / "tok_score_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <type_traits>
using suffix_array::TokenIndex;
typedef TokenIndex::Tokens Tok;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::uint8_t> U8;
static_assert(std::is_same<TokenIndex::Score, suffix_array::DocumentIndex::Score>::value, "the existing Score");
int main() {
    const Tok t{256, 1, 256, 1, 2};
    const Tok q{7, 256, 1, 256};
    TokenIndex ix(t.data(), t.size());                                // the array is built on the device
    const TokenIndex::Score r = ix.infgram_score(q, 1, 4);
    if (r.size() != 4) return 1;
    if (r.s != U32{0, 0, 1, 2} || r.lo != U32{0, 0, 4, 4} || r.hi != U32{6, 6, 6, 6} || r.at_end != U8{1, 1, 0, 0}) return 2;
    if (r.nlo != U32{4, 4, 4, 5} || r.nhi != U32{4, 6, 6, 6}) return 3;
    if (r.count(0) != 0 || r.total(0) != 5 || r.count(1) != 2 || r.total(1) != 5 || r.count(3) != 1 || r.total(3) != 2) return 4;
    const auto r3 = ix.infgram_score(q, 3, 4);                        // {256} occurs twice
    if (r3.s != U32{0, 0, 0, 0}) return 5;
    const auto d = ix.infgram_score(q, 1, 4, {0, 2, 2, 4});           // documents {7, 256}, {}, {1, 256}: no context at position 2
    if (d.s != U32{0, 0, 0, 1} || d.lo != U32{0, 0, 0, 1} || d.hi != U32{6, 6, 6, 3} || d.nlo[3] != 2 || d.nhi[3] != 3) return 6;
    const U32 want{5, 3, 1, 4, 2, 0};
    TokenIndex given(t.data(), t.size(), want.data());
    const auto g = given.infgram_score(q);                            // the defaults: min_count 1, the longest context
    if (g.s != r.s || g.nlo != r.nlo || g.nhi != r.nhi) return 7;
    if (ix.infgram_score(Tok{}).size() != 0) return 8;
    try { ix.infgram_score(q, 0); return 9; } catch (const std::invalid_argument &) { }
    try { ix.infgram_score(q, 1, 0); return 10; } catch (const std::invalid_argument &) { }
    try { ix.infgram_score(q, 1, 4097); return 11; } catch (const std::invalid_argument &) { }
    try { ix.infgram_score(q, 1, 4, {0, 3}); return 12; } catch (const std::invalid_argument &) { }
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "tok_score_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
