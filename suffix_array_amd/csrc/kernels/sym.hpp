// kernels/sym.hpp -- the symbol-generic core of every query over a suffix array (DESIGN.md sections 8f, 11, 21, 23): a text is an
// array of Sym (uint8_t bytes, uint16_t tokens, or token ids below 2^24 in uint32_t), and the comparison of a suffix with a pattern, the match range by two lower
// bounds and the probe of the symbol behind a context are written once over Sym.  Every function is executed by a whole wave
// (gfx950, wave64); an SA entry is added to its offset in 64 bits and checked against n before T is read through it.
#pragma once
#include "common.hpp"

namespace sa {

// the supported symbol types; a uint32_t text holds ids below 2^24 (its owner checks that on the device,
// and every pattern on the host), so a symbol and the sentinel behind the alphabet fit an int
template <typename Sym> constexpr bool sym_supported()
{
    return std::is_same<Sym, uint8_t>::value || std::is_same<Sym, uint16_t>::value || std::is_same<Sym, uint32_t>::value;
}

// the "symbol" of a slot whose suffix ends at the context: sorts behind every symbol (NG_END, TK_END)
template <typename Sym> constexpr int sym_end()
{
    static_assert(sym_supported<Sym>(), "bytes, 16-bit tokens, or token ids below 2^24 in 32 bits");
    return sizeof(Sym) == 4 ? 1 << 24 : 1 << (8 * sizeof(Sym));
}

struct SuffixCmp { int ord; uint32_t lcp; };   // ord: -1 suffix < pattern, 0 equal, +1 suffix > pattern
struct NgRange { uint32_t lo, hi; };

// Rust slice ordering of s[p..] against pat (lexicographic, a proper prefix is smaller) and their lcp, 64 symbols a step: lane l
// compares symbol c + l of both, a ballot finds the first difference.  From symbol c0 on: the caller knows that they agree on
// their first c0 symbols.  *symbols grows by the symbols of every chunk loaded.  Reads only T[p + c0 .. min(n, p + plen)) and
// pat[c0 .. plen).  The symbols travel through the shuffle as int: every supported symbol is below 2^24 (sym_end).
template <typename Sym>
__device__ __forceinline__ SuffixCmp wave_compare_from(const Sym *__restrict__ T, int64_t n, int64_t p, const Sym *__restrict__ pat,
                                                       int64_t plen, int64_t c0, int64_t *symbols)
{
    const int l = lane_id();
    const int64_t slen = n - p;
    int64_t common = slen < plen ? slen : plen;
    if (common < 0) common = 0;                              // (an entry > n: only when the array is not a suffix array)
    for (int64_t c = c0; c < common; c += WAVE) {
        const int64_t i = c + l;
        const bool in = i < common;
        const Sym x = in ? T[p + i] : 0, y = in ? pat[i] : 0;
        *symbols += common - c < WAVE ? common - c : WAVE;
        const uint64_t diff = __ballot(in && x != y);
        if (diff) {
            const int first = __ffsll((unsigned long long)diff) - 1;
            const int xv = __shfl((int)x, first, WAVE), yv = __shfl((int)y, first, WAVE);
            SuffixCmp r; r.ord = xv < yv ? -1 : 1; r.lcp = (uint32_t)(c + first);
            return r;
        }
    }
    SuffixCmp r; r.lcp = (uint32_t)common;
    r.ord = slen < plen ? -1 : (slen > plen ? 1 : 0);
    return r;
}

// The match range of pat[0 .. plen) inside the slots [lo, hi), which hold every suffix that starts with pat and, below and
// above them, only smaller and larger ones: search_all of reference src/sa.rs:182-201.
template <typename Sym>
__device__ __forceinline__ NgRange plain_range(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, int64_t lo, int64_t hi,
                                               const Sym *__restrict__ pat, int64_t plen, int64_t *symbols)
{
    int64_t lo2, hi2 = hi;
    while (lo < hi) {                                         // src/sa.rs:182-190: first i whose suffix is not smaller than pat
        const int64_t m = lo + (hi - lo) / 2;
        if (wave_compare_from(T, n, (int64_t)SA[m], pat, plen, 0, symbols).ord < 0) lo = m + 1; else hi = m;
    }
    lo2 = lo;
    while (lo2 < hi2) {                                       // src/sa.rs:192-201: first j >= i whose suffix does not start with pat
        const int64_t m = lo2 + (hi2 - lo2) / 2;
        if ((int64_t)wave_compare_from(T, n, (int64_t)SA[m], pat, plen, 0, symbols).lcp == plen) lo2 = m + 1; else hi2 = m;
    }
    NgRange r;
    r.lo = (uint32_t)lo; r.hi = (uint32_t)lo2;
    return r;
}

// the symbol behind the context of p symbols of slot i < n + 1, sym_end where the suffix ends at or before it ((int) keeps the
// value: ids are below 2^24)
template <typename Sym>
__device__ __forceinline__ int next_symbol(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, int64_t p, uint32_t i)
{
    const int64_t s = (int64_t)SA[i] + p;
    return s < n ? (int)T[s] : sym_end<Sym>();
}

}  // namespace sa
