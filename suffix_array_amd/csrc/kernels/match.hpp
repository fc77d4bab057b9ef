// kernels/match.hpp -- matching statistics of a query text against a device-resident text and its suffix array (DESIGN.md
// section 15).  Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// T has n bytes, SA n + 1 entries (SA[0] = n); Q has m bytes, C >= 1 is the cap.  For query position j the window is
// w = Q[j .. j + c), c = min(C, m - j); i = the number of slots whose suffix is smaller than w in slice order (1 <= i <= n + 1),
// a = lcp(w, suffix of slot i - 1), b = lcp(w, suffix of slot i) (-1 when i = n + 1); ML[j] = max(a, b), POS[j] = SA[i - 1] if
// a > b else SA[i], MATCH_NONE when ML[j] = 0.
//   k_match_tile<G>  a workgroup owns MATCH_TILE consecutive positions and stages Q[tile .. tile + MATCH_TILE + cap) in LDS once;
//                    G lanes serve one position: lower-bound binary search that keeps l = lcp(w, suffix of slot lo - 1) and
//                    r = lcp(w, suffix of slot hi) and compares from min(l, r) on, four bytes a lane; a and b are the final
//                    l and r (a neighbour the search never probed -- possible only when it started from a bucket -- is compared
//                    once more).  A position with c > cap one of whose compares reaches cap equal bytes is appended to the long
//                    list instead and gets no output here.
//   k_match_long<E>  one wave per listed position, the window read from Q: E = 1 the descent over the LCP table of the search
//                    tree (kernels/esa.hpp), E = 0 the same binary search with 64-byte wave compares.
// The flags of the shared spans (ML == C) go through the span passes of kernels/repeats.hpp (mode KEEP_FIRST: reach = j + C).
// A wrong permutation gives unspecified answers; every entry of SA is checked against n before it is used, every slot taken from
// the bucket table is clamped to 1 .. n + 1 and every load of T or Q is guarded by the array's ends.
#pragma once
#include "sym.hpp"
#include "esa.hpp"
#include "lcp.hpp"

namespace sa {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_TILE = 256;                         // query positions per workgroup
constexpr int MATCH_STAGE_MAX = 4096;                   // window bytes the group path stages at most: a larger cap acts as this one
constexpr int MATCH_CAP_DEFAULT = 64;                   // sa_amd_match_set_group_cap
constexpr int MATCH_CAP_MAX = 1 << 20;
constexpr uint32_t MATCH_NONE = 0xffffffffu;
static_assert(MATCH_THREADS == LCP_THREADS, "the counters use lcp_block_add");

// control words (uint64) at the start of the work block; the span passes' REP_C_* words sit MATCH_C_WORDS behind them
constexpr int MATCH_C_LONG = 0, MATCH_C_BYTES = 1, MATCH_C_STEPS = 2, MATCH_C_MATCHED = 3, MATCH_C_SUM = 4, MATCH_C_BEST = 5, MATCH_C_WORDS = 8;

struct __attribute__((packed, aligned(4))) MatchPair { uint32_t x, y; };      // two words by one 4-byte aligned 8-byte load

// the aligned word at a of the bytes [beg, end): whole when it lies inside, else byte by byte (bytes outside read as 0)
__device__ __forceinline__ uint32_t match_aligned_word(uintptr_t a, uintptr_t beg, uintptr_t end)
{
    if (a >= beg && a + 4 <= end) return *(const uint32_t *)a;
    uint32_t w = 0;
    for (int k = 0; k < 4; ++k)
        if (a + k >= beg && a + k < end) w |= (uint32_t)(*(const uint8_t *)(a + k)) << (8 * k);
    return w;
}

// the four bytes from address x on (any alignment), little-endian; nothing outside [beg, end) is read
__device__ __forceinline__ uint32_t match_word(uintptr_t x, uintptr_t beg, uintptr_t end)
{
    const uintptr_t a = x & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)(x & 3u) * 8u;
    uint32_t w0, w1;
    if (a >= beg && a + 8 <= end) { const MatchPair q = *(const MatchPair *)a; w0 = q.x; w1 = q.y; }
    else { w0 = match_aligned_word(a, beg, end); w1 = match_aligned_word(a + 4, beg, end); }
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
}

// the four bytes from byte offset b of the staged words on
__device__ __forceinline__ uint32_t match_lds_word(const uint32_t *s_w, uint32_t b)
{
    const uint32_t w0 = s_w[b >> 2], w1 = s_w[(b >> 2) + 1];
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> ((b & 3u) * 8u));
}

// The compare of two little-endian 32-bit words that hold 4 / sizeof(Sym) symbols each and differ in the bits d != 0: the index
// of the first differing SYMBOL of the word and *less = the text's symbol there is the smaller VALUE.  With 16-bit tokens the
// lowest differing byte does not decide: 0x0102 against 0x0201 differs first in a byte that says "greater".  A 32-bit symbol is
// the whole word: index 0, compared by value.
template <typename Sym>
__device__ __forceinline__ int match_word_diff(uint32_t d, uint32_t tw, uint32_t qw, bool *less)
{
    if constexpr (sizeof(Sym) == 4) {
        *less = tw < qw;
        return 0;
    } else {
        constexpr uint32_t BITS = 8u * sizeof(Sym), MASK = (1u << BITS) - 1u;
        const int si = (__ffs(d) - 1) >> (sizeof(Sym) == 1 ? 3 : 4);
        *less = ((tw >> (BITS * si)) & MASK) < ((qw >> (BITS * si)) & MASK);
        return si;
    }
}

// the bits of a word that hold its first v symbols, 0 < v < 4 / sizeof(Sym) (a word of one symbol has no partial tail)
template <typename Sym>
__device__ __forceinline__ uint32_t match_tail_mask(int64_t v)
{
    if constexpr (sizeof(Sym) == 4) return 0xffffffffu;
    else return (1u << (8u * (uint32_t)sizeof(Sym) * (uint32_t)v)) - 1u;
}

// lcp of T[p ..] and the window at BYTE offset wb of the staged words, both known to agree on [0, from) and compared on
// [from, limit) -- offsets and lengths in symbols: the G lanes of a group take one 32-bit word each, W = 4 / sizeof(Sym) symbols,
// W G symbols a round.  limit <= n - p.  Returns limit when nothing differs, else the offset of the first difference and *less =
// the text's symbol is the smaller one.  *symbols grows by W G a round.
template <int G, typename Sym>
__device__ __forceinline__ int64_t match_group_lcp(const Sym *__restrict__ T, int64_t n, int64_t p, const uint32_t *s_w, uint32_t wb,
                                                   int64_t from, int64_t limit, int gl, int gshift, unsigned long long *symbols, bool *less)
{
    constexpr int W = 4 / (int)sizeof(Sym);
    static_assert(sizeof(Sym) == 1 || sizeof(Sym) == 2 || sizeof(Sym) == 4, "a word holds whole symbols");
    const uintptr_t beg = (uintptr_t)T, end = (uintptr_t)(T + n);
    for (int64_t off = from; off < limit; off += W * G) {
        const int64_t o = off + W * gl;
        uint32_t d = 0, tw = 0, qw = 0;
        if (o < limit) {
            tw = match_word((uintptr_t)(T + p + o), beg, end);
            qw = match_lds_word(s_w, wb + (uint32_t)sizeof(Sym) * (uint32_t)o);
            const int64_t v = limit - o;                           // symbols left: the tail of a word is masked in symbols
            d = (tw ^ qw) & (v >= W ? 0xffffffffu : match_tail_mask<Sym>(v));
        }
        *symbols += W * G;
        const uint32_t gm = (uint32_t)(__ballot(d != 0) >> gshift) & ((1u << G) - 1u);
        if (gm) {
            const int f = __ffs(gm) - 1;
            const uint32_t df = __shfl(d, gshift + f, WAVE), tf = __shfl(tw, gshift + f, WAVE), qf = __shfl(qw, gshift + f, WAVE);
            return off + W * f + match_word_diff<Sym>(df, tf, qf, less);
        }
    }
    return limit;
}

// ge: the effective cap of the group path, min(group cap, MATCH_STAGE_MAX); dynamic LDS: match_stage_words(ge) words.
// ML, POS, flag: any of them may be nullptr.  bkt: the bucket table or nullptr.
__host__ __device__ inline int match_stage_words(int ge) { return (3 + MATCH_TILE + ge + 3) / 4 + 2; }

template <int G>
__global__ __launch_bounds__(MATCH_THREADS) void k_match_tile(
    const uint8_t *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ bkt,
    const uint8_t *__restrict__ Q, int64_t m, int64_t C, int ge, uint32_t *__restrict__ ML, uint32_t *__restrict__ POS,
    uint8_t *__restrict__ flag, uint32_t *__restrict__ long_list, unsigned long long *__restrict__ ctl)
{
    extern __shared__ uint32_t s_w[];
    constexpr int GROUPS = MATCH_THREADS / G;
    static_assert(G == 4 || G == 8 || G == 16, "a group is a power of two of lanes inside one wave");
    const int64_t tile0 = (int64_t)blockIdx.x * MATCH_TILE;
    {   // the staged bytes mirror Q's alignment: word k is the aligned word at a0 + 4 k
        const uintptr_t qbeg = (uintptr_t)Q, qend = (uintptr_t)(Q + m);
        const uintptr_t a0 = (uintptr_t)(Q + tile0) & ~(uintptr_t)3;
        const int words = match_stage_words(ge);
        for (int k = threadIdx.x; k < words; k += MATCH_THREADS) s_w[k] = match_aligned_word(a0 + 4 * (uintptr_t)k, qbeg, qend);
    }
    __syncthreads();
    const uint32_t sh0 = (uint32_t)((uintptr_t)(Q + tile0) & 3u);
    const int gl = (int)threadIdx.x & (G - 1), gi = (int)threadIdx.x / G, gshift = lane_id() & ~(G - 1);
    const int64_t N = n + 1;
    unsigned long long bytes = 0, steps = 0, matched = 0, sum = 0, best = 0;
    for (int it = 0; it < MATCH_TILE / GROUPS; ++it) {
        const int64_t j = tile0 + (int64_t)it * GROUPS + gi;
        bool is_long = false;
        if (j < m) {
            const int64_t c = C < m - j ? C : m - j;
            const bool capped = c > (int64_t)ge;               // a compare that reaches ge equal bytes sends the position to pass 2
            const uint32_t wb = sh0 + (uint32_t)(j - tile0);
            // slots below lo hold smaller suffixes, slots from hi on do not; slot 0 is the empty suffix: a = 0 there
            int64_t lo = 1, hi = N, l = 0, r = 0;
            bool lp = true, rp = false;                         // l / r are the exact lcp of slot lo - 1 / hi (hi = N: no such slot)
            if (bkt) {
                // every suffix of the window's bucket shares its first two bytes (one byte for c = 1), every suffix below the
                // bucket is smaller and every one above it larger: the insertion point lies in [lo, hi], also when lo == hi
                const uint32_t w2 = match_lds_word(s_w, wb);
                const int c0 = (int)(w2 & 255u), c1 = (int)((w2 >> 8) & 255u);
                if (c > 1) { lo = bkt[c0 * 257 + c1 + 1]; hi = bkt[c0 * 257 + c1 + 2]; l = r = 2; }
                else { lo = bkt[c0 * 257]; hi = bkt[c0 * 257 + 257]; l = r = 1; }
                if (lo < 1) lo = 1;
                if (hi > N) hi = N;
                if (hi < lo) hi = lo;
                lp = rp = false;
            }
            // compares the suffix of `slot` with the window from byte `from` on; false: the position goes to pass 2
            auto probe = [&](int64_t slot, int64_t from, int64_t *lcp, bool *smaller) -> bool {
                ++steps;
                if (capped && from >= (int64_t)ge) return false;
                const int64_t p = (int64_t)SA[slot];
                int64_t common = n - p < c ? n - p : c;
                if (common < from) common = from;                 // (only when the array is not the suffix array)
                if (p > n) common = 0;
                const int64_t limit = capped && common > (int64_t)ge ? (int64_t)ge : common;
                bool less = false;
                const int64_t v = p > n ? 0 : match_group_lcp<G>(T, n, p, s_w, wb, from < limit ? from : limit, limit, gl, gshift, &bytes, &less);
                if (capped && v >= (int64_t)ge) return false;
                *lcp = v;
                *smaller = v < limit ? less : common < c;         // equal to the end: a proper prefix of the window is smaller
                return true;
            };
            if (ge == 0) is_long = true;
            while (!is_long && lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                int64_t v = 0;
                bool smaller = false;
                if (!probe(mid, l < r ? l : r, &v, &smaller)) { is_long = true; break; }
                if (smaller) { lo = mid + 1; l = v; lp = true; } else { hi = mid; r = v; rp = true; }
            }
            int64_t a = l, b = -1;
            if (!is_long && !lp) {
                bool unused;
                if (!probe(lo - 1, 0, &a, &unused)) is_long = true;
            }
            if (!is_long && lo <= n) {
                b = r;
                bool unused;
                if (!rp && !probe(lo, 0, &b, &unused)) is_long = true;
            }
            if (!is_long && gl == 0) {
                const int64_t ml = a > b ? a : b;
                if (ML) ML[j] = (uint32_t)ml;
                if (POS) POS[j] = ml == 0 ? MATCH_NONE : (a > b ? SA[lo - 1] : SA[lo]);
                if (flag) flag[j] = ml == C ? 1 : 0;
                if (ml > 0) {
                    ++matched;
                    sum += (unsigned long long)ml;
                    const unsigned long long key = ((unsigned long long)ml << 32) | (uint32_t)~(uint32_t)j;
                    best = best > key ? best : key;
                }
            }
        }
        const int64_t at = lcp_wave_append(is_long && gl == 0, (uint32_t *)&ctl[MATCH_C_LONG]);
        if (at >= 0) long_list[at] = (uint32_t)j;
    }
    if (gl != 0) { bytes = 0; steps = 0; }                      // (the lanes of a group count the same)
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long b2 = __shfl_xor(best, o, WAVE);
        best = best > b2 ? best : b2;
    }
    if (lane_id() == 0 && best) atomicMax(&ctl[MATCH_C_BEST], best);
    lcp_block_add(bytes, &ctl[MATCH_C_BYTES]);
    lcp_block_add(steps, &ctl[MATCH_C_STEPS]);
    lcp_block_add(matched, &ctl[MATCH_C_MATCHED]);
    lcp_block_add(sum, &ctl[MATCH_C_SUM]);
}

// One wave per entry of the long list.  ESA: pair / log_p are the LCP table of the search tree and its depth.
template <bool ESA>
__global__ __launch_bounds__(MATCH_THREADS) void k_match_long(
    const uint8_t *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint64_t *__restrict__ pair, int log_p,
    const uint8_t *__restrict__ Q, int64_t m, int64_t C, const uint32_t *__restrict__ long_list, int64_t count,
    uint32_t *__restrict__ ML, uint32_t *__restrict__ POS, uint8_t *__restrict__ flag, unsigned long long *__restrict__ ctl)
{
    const int64_t q = ((int64_t)blockIdx.x * MATCH_THREADS + threadIdx.x) / WAVE;
    if (q >= count) return;                                     // whole waves leave together
    const int64_t j = (int64_t)long_list[q];
    if (j >= m) return;
    const int64_t c = C < m - j ? C : m - j;
    const uint8_t *pat = Q + j;
    int64_t bytes = 0, steps = 0, i, a, b;
    if (ESA) {
        int64_t table_steps = 0;
        const EsaState st = esa_descent<false>(T, SA, n, pair, log_p, pat, c, &bytes, &table_steps);
        steps = log_p;
        i = (int64_t)st.L;
        a = i >= 1 ? st.l : -1;
        b = i <= n ? st.r : -1;
    } else {
        int64_t lo = 1, hi = n + 1, l = 0, r = 0;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            const SuffixCmp s = wave_compare_from(T, n, (int64_t)SA[mid], pat, c, l < r ? l : r, &bytes);
            ++steps;
            if (s.ord < 0) { lo = mid + 1; l = s.lcp; } else { hi = mid; r = s.lcp; }
        }
        i = lo; a = l; b = i <= n ? r : -1;
    }
    if (lane_id() != 0) return;
    const int64_t ml = a > b ? a : b;
    uint32_t pos = MATCH_NONE;
    if (ml > 0 && i <= n + 1) pos = a > b ? SA[i - 1] : SA[i];
    if (ML) ML[j] = (uint32_t)(ml > 0 ? ml : 0);
    if (POS) POS[j] = pos;
    if (flag) flag[j] = ml == C ? 1 : 0;
    atomicAdd(&ctl[MATCH_C_BYTES], (unsigned long long)bytes);
    atomicAdd(&ctl[MATCH_C_STEPS], (unsigned long long)steps);
    if (ml > 0) {
        atomicAdd(&ctl[MATCH_C_MATCHED], 1ull);
        atomicAdd(&ctl[MATCH_C_SUM], (unsigned long long)ml);
        atomicMax(&ctl[MATCH_C_BEST], ((unsigned long long)ml << 32) | (uint32_t)~(uint32_t)j);
    }
}

}  // namespace sa
