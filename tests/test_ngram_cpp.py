"""A C++ caller of the n-gram methods of suffix_array::DocumentIndex (include/suffix_array_amd.hpp): the example of the header's
section on n-gram and infinity-gram queries, through the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_document_index(tmp_path):
    src = tmp_path / "ngram_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::DocumentIndex;
typedef std::vector<std::uint32_t> U32;
typedef std::vector<std::pair<std::uint8_t, std::uint32_t>> Next;
int main() {
    const char *txt = "abracadabra";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    const std::size_t n = std::strlen(txt);
    DocumentIndex ix(t, n, U32{0, 11});                               // the array is built on the device
    const auto nb = ix.next_bytes({"a", "abra", "", "x"});
    if (nb.size() != 4) return 1;
    if (nb[0].lo != 1 || nb[0].hi != 6 || !nb[0].at_end || nb[0].next != Next{{'b', 2}, {'c', 1}, {'d', 1}}) return 2;
    if (nb[1].lo != 2 || nb[1].hi != 4 || !nb[1].at_end || nb[1].next != Next{{'c', 1}}) return 3;
    if (nb[2].lo != 0 || nb[2].hi != 12 || !nb[2].at_end || nb[2].next != Next{{'a', 5}, {'b', 2}, {'c', 1}, {'d', 1}, {'r', 2}}) return 4;
    if (nb[3].lo != nb[3].hi || nb[3].at_end || !nb[3].next.empty()) return 5;
    for (const auto &r : nb) {                                        // sum(next) + at_end == hi - lo
        std::uint32_t sum = r.at_end ? 1 : 0;
        for (const auto &e : r.next) sum += e.second;
        if (sum != r.hi - r.lo) return 6;
    }
    auto g = ix.infgram({"xcabra"});
    if (g.size() != 1 || g[0].suffix_len != 4 || g[0].lo != 2 || g[0].hi != 4 || g[0].next != Next{{'c', 1}}) return 7;
    g = ix.infgram({"xcabra"}, 2);
    if (g[0].suffix_len != 4 || g[0].lo != 2 || g[0].hi != 4) return 8;
    g = ix.infgram({"xcabra", "zz", ""}, 3);
    if (g[0].suffix_len != 1 || g[0].lo != 1 || g[0].hi != 6 || g[0].next != nb[0].next) return 9;
    if (g[1].suffix_len != 0 || g[1].lo != 0 || g[1].hi != 12 || g[1].next != nb[2].next || g[2].next != nb[2].next) return 10;
    g = ix.infgram({"xcabra"}, 1, 2);
    if (g[0].suffix_len != 2 || g[0].lo != 10 || g[0].hi != 12 || !g[0].at_end || g[0].next != Next{{'c', 1}}) return 11;
    try { ix.infgram({"a"}, 0); return 12; } catch (const std::invalid_argument &) { }
    if (!ix.next_bytes({}).empty() || !ix.infgram({}).empty()) return 13;
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "ngram_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
