"""A C++ caller of suffix_array::TokenIndex (include/suffix_array_amd.hpp): the example of the header's section on 16-bit token
texts, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_token_index(tmp_path):
    src = tmp_path / "token_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
using suffix_array::TokenIndex;
typedef TokenIndex::Tokens Tok;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::pair<std::uint16_t, std::uint32_t>> Next;
int main() {
    const Tok t{256, 1, 256, 1, 2};
    const U32 want{5, 3, 1, 4, 2, 0};
    TokenIndex ix(t.data(), t.size());                                // the array is built on the device
    if (ix.len() != 5 || ix.sa() != want) return 1;
    TokenIndex given(t.data(), t.size(), want.data());
    if (given.sa() != want) return 2;
    const auto r = ix.search({Tok{256, 1}, Tok{1}, Tok{}, Tok{9}, Tok{1, 256}});
    if (r[0] != std::make_pair(4u, 6u) || r[1] != std::make_pair(1u, 3u) || r[2] != std::make_pair(0u, 6u) || r[3].first != r[3].second) return 3;
    if (r[4] != std::make_pair(2u, 3u)) return 4;                     // {1, 256}: bytes 00 01 01 00 -- a little-endian image would hold 01 00 00 01
    if (ix.count({Tok{256, 1}, Tok{9}}) != U32{2, 0} || ix.contains({Tok{256}, Tok{3}}) != std::vector<bool>{true, false}) return 5;
    const auto nt = given.next_tokens({Tok{256, 1}, Tok{1}, Tok{2}, Tok{}, Tok{9}});
    if (nt.size() != 5) return 6;
    if (nt[0].lo != 4 || nt[0].hi != 6 || nt[0].at_end || nt[0].next != Next{{2, 1}, {256, 1}}) return 7;
    if (nt[1].lo != 1 || nt[1].hi != 3 || nt[1].at_end || nt[1].next != Next{{2, 1}, {256, 1}}) return 8;
    if (nt[2].lo != 3 || nt[2].hi != 4 || !nt[2].at_end || !nt[2].next.empty()) return 9;
    if (nt[3].lo != 0 || nt[3].hi != 6 || !nt[3].at_end || nt[3].next != Next{{1, 2}, {2, 1}, {256, 2}}) return 10;
    if (nt[4].lo != nt[4].hi || nt[4].at_end || !nt[4].next.empty()) return 11;
    for (const auto &x : nt) {                                        // sum(next) + at_end == hi - lo
        std::uint32_t sum = x.at_end ? 1 : 0;
        for (const auto &e : x.next) sum += e.second;
        if (sum != x.hi - x.lo) return 12;
    }
    auto g = ix.infgram({Tok{7, 256, 1}});
    if (g.size() != 1 || g[0].suffix_len != 2 || g[0].lo != 4 || g[0].hi != 6 || g[0].next != nt[0].next) return 13;
    g = ix.infgram({Tok{7, 256, 1}}, 3);
    if (g[0].suffix_len != 0 || g[0].lo != 0 || g[0].hi != 6 || g[0].next != nt[3].next) return 14;
    g = ix.infgram({Tok{7, 256, 1}}, 2, 1);
    if (g[0].suffix_len != 1 || g[0].lo != 1 || g[0].hi != 3) return 15;
    try { ix.infgram({Tok{1}}, 0); return 16; } catch (const std::invalid_argument &) { }
    if (!ix.next_tokens({}).empty() || !ix.infgram({}).empty() || !ix.search({}).empty()) return 17;
    const U32 bad{5, 3, 1, 4, 2, 9};
    try { TokenIndex b(t.data(), t.size(), bad.data()); return 18; } catch (const std::runtime_error &) { }
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "token_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
