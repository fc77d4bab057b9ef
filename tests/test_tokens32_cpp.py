"""A C++ caller of suffix_array::TokenIndex32 (include/suffix_array_amd.hpp): the example of the header's section on 32-bit
token ids (include/suffix_array_amd_tok32.h), through the mirror, after tests/test_tokens_cpp.py."""
import os
import subprocess

import pytest

from suffix_array_amd import TokenIndex32  # noqa: F401  (nothing here is collected without the feature)
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_token_index32(tmp_path):
    src = tmp_path / "token32_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <type_traits>
using suffix_array::TokenIndex32;
typedef TokenIndex32::Tokens Tok;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::pair<std::uint32_t, std::uint32_t>> Next;
static_assert(std::is_same<TokenIndex32::Token, std::uint32_t>::value, "ids are held in 32 bits");
static_assert(std::is_same<suffix_array::TokenIndex::Token, std::uint16_t>::value, "the 16-bit index is what it was");
int main() {
    const Tok t{65537, 1, 65536, 1, 2};
    const U32 want{5, 3, 1, 4, 2, 0};
    if (sa_amd_max_tokens_u32() != 715827882 || SA_AMD_TOKEN_LIMIT_U32 != 16777216) return 100;
    TokenIndex32 ix(t.data(), t.size());                              // the array is built on the device
    if (ix.len() != 5 || ix.sa() != want) return 1;
    TokenIndex32 given(t.data(), t.size(), want.data());
    if (given.sa() != want) return 2;
    const auto r = ix.search({Tok{65536, 1}, Tok{1}, Tok{}, Tok{9}, Tok{1, 65536}, Tok{1, 0}});
    if (r[0] != std::make_pair(4u, 5u) || r[1] != std::make_pair(1u, 3u) || r[2] != std::make_pair(0u, 6u) || r[3].first != r[3].second) return 3;
    if (r[4] != std::make_pair(2u, 3u)) return 4;
    if (r[5].first != r[5].second) return 19;                         // {1, 0}: what {1, 65536} is once truncated to 16 bits
    if (ix.count({Tok{1}, Tok{9}}) != U32{2, 0} || ix.contains({Tok{65537}, Tok{3}}) != std::vector<bool>{true, false}) return 5;
    const auto nt = given.next_tokens({Tok{65536, 1}, Tok{1}, Tok{2}, Tok{}, Tok{9}});
    if (nt.size() != 5) return 6;
    if (nt[0].lo != 4 || nt[0].hi != 5 || nt[0].at_end || nt[0].next != Next{{2, 1}}) return 7;
    if (nt[1].lo != 1 || nt[1].hi != 3 || nt[1].at_end || nt[1].next != Next{{2, 1}, {65536, 1}}) return 8;
    if (nt[2].lo != 3 || nt[2].hi != 4 || !nt[2].at_end || !nt[2].next.empty()) return 9;
    if (nt[3].lo != 0 || nt[3].hi != 6 || !nt[3].at_end || nt[3].next != Next{{1, 2}, {2, 1}, {65536, 1}, {65537, 1}}) return 10;
    if (nt[4].lo != nt[4].hi || nt[4].at_end || !nt[4].next.empty()) return 11;
    for (const auto &x : nt) {                                        // sum(next) + at_end == hi - lo
        std::uint32_t sum = x.at_end ? 1 : 0;
        for (const auto &e : x.next) sum += e.second;
        if (sum != x.hi - x.lo) return 12;
    }
    auto g = ix.infgram({Tok{7, 65536, 1}});
    if (g.size() != 1 || g[0].suffix_len != 2 || g[0].lo != 4 || g[0].hi != 5 || g[0].next != nt[0].next) return 13;
    g = ix.infgram({Tok{7, 65536, 1}}, 3);
    if (g[0].suffix_len != 0 || g[0].lo != 0 || g[0].hi != 6 || g[0].next != nt[3].next) return 14;
    g = ix.infgram({Tok{7, 65536, 1}}, 2);
    if (g[0].suffix_len != 1 || g[0].lo != 1 || g[0].hi != 3) return 15;
    try { ix.infgram({Tok{1}}, 0); return 16; } catch (const std::invalid_argument &) { }
    if (!ix.next_tokens({}).empty() || !ix.infgram({}).empty() || !ix.search({}).empty()) return 17;
    const U32 bad{5, 3, 1, 4, 2, 9};
    try { TokenIndex32 b(t.data(), t.size(), bad.data()); return 18; } catch (const std::runtime_error &) { }
    const auto sc = ix.infgram_score(Tok{7, 65536, 1, 2}, 1, 4);      // the header's table
    if (sc.s != U32{0, 0, 1, 2} || sc.lo != U32{0, 0, 4, 4} || sc.hi != U32{6, 6, 5, 5}) return 20;
    if (sc.nlo != U32{4, 4, 4, 4} || sc.nhi != U32{4, 5, 5, 5} || sc.at_end != std::vector<std::uint8_t>{1, 1, 0, 0}) return 21;
    const Tok over{1, 1u << 24, 2};                                   // an id that is no token: in the text, in a pattern, in a query
    try { TokenIndex32 b(over.data(), over.size()); return 22; } catch (const std::runtime_error &) { }
    try { TokenIndex32 b(over.data(), over.size(), U32{3, 0, 2, 1}.data()); return 23; } catch (const std::runtime_error &) { }
    try { ix.search({over}); return 24; } catch (const std::runtime_error &) { }
    try { ix.next_tokens({Tok{1}, over}); return 25; } catch (const std::runtime_error &) { }
    try { ix.infgram_score(over); return 26; } catch (const std::runtime_error &) { }
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "token32_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
