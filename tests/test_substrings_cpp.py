"""A C++ caller of repeated_substrings of include/suffix_array_amd.hpp: the example of the header's section on repeated
substrings, through the free function and the SuffixArray method of the mirror."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_program_through_the_mirror(tmp_path):
    src = tmp_path / "substrings_caller.cpp"
    src.write_text(r'''
#include "suffix_array_amd.hpp"
#include <cstdio>
#include <cstring>
using suffix_array::RepeatedSubstring;
using suffix_array::SuffixArray;
typedef std::vector<RepeatedSubstring> Rows;
int main() {
    const char *txt = "banana";
    const auto *t = reinterpret_cast<const std::uint8_t *>(txt);
    const std::size_t n = std::strlen(txt);
    const Rows all = suffix_array::repeated_substrings(t, n);         // the array is built on the device and stays there
    if (all != Rows{{1, 3, 1, 0, 5}, {2, 2, 3, 1, 3}, {5, 2, 2, 0, 4}}) return 1;
    for (const auto &r : all)
        if (r.pos + r.depth > n || r.count < 2 || r.parent >= r.depth) return 2;      // every row's substring can be read at pos
    if (std::memcmp(txt + all[1].pos, "ana", 3) != 0) return 3;
    const SuffixArray s = SuffixArray::new_(t, n);
    if (s.repeated_substrings() != all) return 4;
    if (s.repeated_substrings(1, 0, 2, SA_AMD_SUBSTR_BY_COUNT, 1) != Rows{{1, 3, 1, 0, 5}}) return 5;
    if (s.repeated_substrings(1, 0, 2, SA_AMD_SUBSTR_BY_LENGTH, 2) != Rows{{2, 2, 3, 1, 3}, {5, 2, 2, 0, 4}}) return 6;
    if (suffix_array::repeated_substrings(t, n, 1, 0, 2, SA_AMD_SUBSTR_BY_COVER, 9) != Rows{{2, 2, 3, 1, 3}, {5, 2, 2, 0, 4}, {1, 3, 1, 0, 5}}) return 7;
    if (suffix_array::repeated_substrings(t, n, 1, 1, 2, SA_AMD_SUBSTR_BY_COVER, 9, s.sa().data()) != Rows{{1, 3, 1, 0, 5}, {5, 2, 2, 0, 4}}) return 8;
    if (suffix_array::repeated_substrings(t, n, 1, 0, 3) != Rows{{1, 3, 1, 0, 5}}) return 9;
    if (!suffix_array::repeated_substrings(t, 0).empty() || !suffix_array::repeated_substrings(t, 1).empty()) return 10;
    try { suffix_array::repeated_substrings(t, n, 0); return 11; } catch (const std::invalid_argument &) { }
    try { suffix_array::repeated_substrings(t, n, 3, 2); return 12; } catch (const std::invalid_argument &) { }
    try { suffix_array::repeated_substrings(t, n, 1, 0, 1); return 13; } catch (const std::invalid_argument &) { }
    try { suffix_array::repeated_substrings(t, n, 1, 0, 2, SA_AMD_SUBSTR_BY_COUNT, 0); return 14; } catch (const std::invalid_argument &) { }
    try { suffix_array::repeated_substrings(t, n, 1, 0, 2, 7, 1); return 15; } catch (const std::invalid_argument &) { }
    sa_amd_substr_stats st;
    (void)s.repeated_substrings(2, 3, 2);
    sa_amd_last_substr_stats(&st);
    if (st.nodes != 3 || st.selected != 2 || st.distinct_all != 5 || st.distinct_selected != 3) return 16;     // an, ana, na
    std::puts("ok");
    return 0;
}
''')
    exe = tmp_path / "substrings_caller_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "suffix_array_amd"), "-lsuffix_array_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "suffix_array_amd")])
    assert subprocess.call([str(exe)]) == 0
