// kernels/score.hpp -- scoring a query text under the infinity-gram model: for every position j of the
// query the longest context Q[j - s .. j) that occurs at least min_count times in the indexed text (the back-off of
// kernels/ngram.hpp, run backwards from every position), its range, and the sub-range of the context followed by Q[j].
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// Every kernel is a template over Sym (kernels/sym.hpp): uint8_t bytes for the byte index, uint16_t and uint32_t tokens for the
// token indexes (DESIGN.md sections 24 and 25).  Lengths, offsets, ge, max_len and q_off count symbols; a byte address is sizeof(Sym) times as far.
// T has n symbols, SA n + 1 slots; Q has m symbols in documents q_off[0 .. ndocs] (nullptr: one document).  For position j of the
// document that starts at `start`: cap = min(j - start, max_len), S[j] = the largest s in 0 .. cap whose range has at least
// min_count slots.  The count never grows with s: the length is found by galloping (s = 1, 2, 4, ... clamped to cap, until a
// probe fails or cap holds) and a bisection between the last good and the first bad length.
//   k_score_tile<G>  a workgroup owns SCORE_TILE consecutive positions and stages Q[tile0 - ge .. tile0 + SCORE_TILE) in LDS
//                    once; G lanes serve one position.  A range search is two binary searches by the group, the pattern in
//                    LDS, started from the bigram bucket where there is a table (bytes only), each compare from the symbols both
//                    ends of the interval are known to share.  A position whose gallop reaches ge good with cap > ge is appended
//                    to the long list with the range of its ge symbols and gets no output here.
//   k_score_long     one wave per listed position, the context read from Q: the gallop goes on behind ge with ngram_range.
// Both end the same way: at_end from slot LO, then two lower bounds on the symbol behind the context inside [LO + at_end, HI).
// A wrong permutation gives unspecified answers; every slot read lies in [0, n + 1), every SA entry is checked against n
// before T is read through it, and Q is read inside [0, m) only.
#pragma once
#include "sym.hpp"
#include "match.hpp"
#include "ngram.hpp"

namespace sa {

constexpr int SCORE_THREADS = MATCH_THREADS;
constexpr int SCORE_TILE = 256;                         // query positions per workgroup
constexpr int SCORE_G = 8;                              // lanes that serve one position
constexpr int SCORE_STAGE_MAX = 4096;                   // SA_AMD_SCORE_MAX_CONTEXT: the context symbols a tile stages at most
constexpr int SCORE_CAP_DEFAULT = 64;                   // sa_amd_score_set_group_cap
constexpr int SCORE_CAP_MAX = 1 << 20;
static_assert(SCORE_THREADS == LCP_THREADS, "the counters use lcp_block_add");

// the control words of a call (unsigned long long each)
enum { SC_W_LONG = 0, SC_W_GROUP_SEARCHES, SC_W_LONG_SEARCHES, SC_W_LOOKUPS, SC_W_BYTES, SC_W_ZERO, SC_W_COUNT };

// dynamic LDS of k_score_tile: the aligned words that cover ge + SCORE_TILE symbols at any alignment, two more for match_lds_word
template <typename Sym>
__host__ __device__ inline int score_stage_words(int ge) { return (3 + (int)sizeof(Sym) * (ge + SCORE_TILE) + 3) / 4 + 2; }

// the bits of a staged word that are the symbol at its start: the whole word for a 4-byte symbol
template <typename Sym> constexpr uint32_t score_sym_mask() { return sizeof(Sym) == 4 ? 0xffffffffu : (1u << (8 * (sizeof(Sym) & 3))) - 1u; }

// The document of position j < m: *next = the first entry of q_off above j (m where there is none), returns the entry before
// it, the document's start.  Whatever q_off holds, 0 <= start <= j.
__device__ __forceinline__ int64_t score_doc_start(const int64_t *__restrict__ q_off, int64_t ndocs, int64_t m, int64_t j, int64_t *next)
{
    int64_t lo = 1, hi = ndocs + 1;                             // the first d in 1 .. ndocs with q_off[d] > j
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (q_off[mid] <= j) lo = mid + 1; else hi = mid;
    }
    *next = lo <= ndocs ? q_off[lo] : m;
    int64_t start = q_off[lo - 1];
    if (start < 0) start = 0;
    if (start > j) start = j;
    return start;
}

// The match range of the s >= 1 symbols at BYTE offset wb of the staged words, by a group of G lanes: the first slot whose suffix
// is not smaller than the pattern, then the first one behind it that does not start with the pattern.  l / r: symbols that the
// suffixes below lo / from hi on share with the pattern -- every slot between them shares min(l, r).  bkt: the bigram bucket
// table, bytes only (any other Sym: that branch is compiled out and the caller passes nullptr).
template <int G, typename Sym>
__device__ __forceinline__ NgRange score_group_range(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n,
                                                     const uint32_t *__restrict__ bkt, const uint32_t *s_w, uint32_t wb, int64_t s, int gl,
                                                     int gshift, unsigned long long *symbols)
{
    const int64_t N = n + 1;
    int64_t lo = 0, hi = N, l = 0, r = 0;
    if constexpr (std::is_same<Sym, uint8_t>::value) {
        if (bkt) {
            const uint32_t w2 = match_lds_word(s_w, wb);
            const int c0 = (int)(w2 & 255u), c1 = (int)((w2 >> 8) & 255u);
            if (s > 1) { lo = bkt[c0 * 257 + c1 + 1]; hi = bkt[c0 * 257 + c1 + 2]; l = r = 2; }
            else { lo = bkt[c0 * 257]; hi = bkt[c0 * 257 + 257]; l = r = 1; }
            if (hi > N) hi = N;
            if (lo > hi) lo = hi;
        }
    }
    const int64_t top = hi, shared = r;
    // lcp of the pattern and the suffix of `slot`, compared from `from` on; *smaller: the suffix sorts below the pattern
    auto probe = [&](int64_t slot, int64_t from, bool *smaller) -> int64_t {
        const int64_t p = (int64_t)SA[slot];
        int64_t common = n - p < s ? n - p : s;
        if (common < from) common = from;                         // (only when the array is not the suffix array)
        if (p > n) common = 0;
        bool less = false;
        const int64_t v = p > n ? 0 : match_group_lcp<G>(T, n, p, s_w, wb, from < common ? from : common, common, gl, gshift, symbols, &less);
        *smaller = v < common ? less : common < s;                // equal to its end: a proper prefix of the pattern is smaller
        return v;
    };
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        bool smaller = false;
        const int64_t v = probe(mid, l < r ? l : r, &smaller);
        if (smaller) { lo = mid + 1; l = v; } else { hi = mid; r = v; }
    }
    // from lo on no suffix is smaller, those that start with the pattern come first and the shared symbols never grow again
    int64_t lo2 = lo, hi2 = top, r2 = shared;
    while (lo2 < hi2) {
        const int64_t mid = lo2 + ((hi2 - lo2) >> 1);
        bool unused = false;
        const int64_t v = probe(mid, r2, &unused);
        if (v == s) lo2 = mid + 1; else { hi2 = mid; r2 = v; }
    }
    NgRange out;
    out.lo = (uint32_t)lo; out.hi = (uint32_t)lo2;
    return out;
}

// the first slot of [lo, hi) whose symbol behind a context of `depth` symbols is not below `target` (sym_end<Sym>() sorts behind
// every symbol and is a target itself: the upper bound of the largest symbol)
template <typename Sym>
__device__ __forceinline__ uint32_t score_byte_bound(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, int64_t depth,
                                                     uint32_t lo, uint32_t hi, int target, uint32_t *probes)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        ++*probes;
        if (next_symbol(T, SA, n, depth, mid) < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct ScoreOut { uint32_t *S, *LO, *HI; uint8_t *AT_END; uint32_t *NLO, *NHI; };      // any of them may be nullptr

// The end of a position whose context of s symbols has the range [lo, hi) and whose own symbol is `sym`: lanes `first` and
// `first + 1` of the wave, both active, run one lower bound each, for sym and sym + 1 (`odd` tells them apart); every caller lane
// gets the answers and lane `first` writes.  Returns 1 on lane `first` where the continuation does not occur.
template <typename Sym>
__device__ __forceinline__ uint32_t score_finish(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, int64_t j, int64_t s,
                                                 uint32_t lo, uint32_t hi, int sym, int first, bool odd, const ScoreOut &o, uint32_t *probes)
{
    const uint32_t N1 = (uint32_t)n + 1u;
    if (hi > N1) hi = N1;
    if (lo > hi) lo = hi;
    const uint32_t ae = hi > lo && (int64_t)SA[lo] + s >= n ? 1u : 0u;
    const uint32_t at = score_byte_bound(T, SA, n, s, lo + ae, hi, sym + (odd ? 1 : 0), probes);
    const uint32_t nlo = (uint32_t)__shfl((int)at, first, WAVE), nhi = (uint32_t)__shfl((int)at, first + 1, WAVE);
    if (lane_id() != first) return 0;
    if (o.S) o.S[j] = (uint32_t)s;
    if (o.LO) o.LO[j] = lo;
    if (o.HI) o.HI[j] = hi;
    if (o.AT_END) o.AT_END[j] = (uint8_t)ae;
    if (o.NLO) o.NLO[j] = nlo;
    if (o.NHI) o.NHI[j] = nhi;
    return nhi == nlo ? 1u : 0u;
}

// ge: the effective cap of the group path, min(group cap, max_len, SCORE_STAGE_MAX); dynamic LDS: score_stage_words<Sym>(ge)
// words.  The long list is three arrays of m entries: the position and the range of its last ge symbols.  Q is aligned to Sym.
template <int G, typename Sym>
__global__ __launch_bounds__(SCORE_THREADS) void k_score_tile(
    const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ bkt,
    const Sym *__restrict__ Q, int64_t m, const int64_t *__restrict__ q_off, int64_t ndocs, uint32_t min_count, int64_t max_len, int ge,
    ScoreOut out, uint32_t *__restrict__ long_list, uint32_t *__restrict__ long_lo, uint32_t *__restrict__ long_hi,
    unsigned long long *__restrict__ ctl)
{
    extern __shared__ uint32_t s_w[];
    __shared__ int64_t s_doc[2];
    constexpr int GROUPS = SCORE_THREADS / G;
    static_assert(G == 4 || G == 8 || G == 16, "a group is a power of two of lanes inside one wave");
    const int64_t tile0 = (int64_t)blockIdx.x * SCORE_TILE;
    constexpr uint32_t SB = (uint32_t)sizeof(Sym);
    const uintptr_t q0 = (uintptr_t)Q + (uintptr_t)((int64_t)SB * (tile0 - (int64_t)ge));   // the address of Q[tile0 - ge]: below Q in the first tiles
    {   // the staged bytes mirror Q's alignment (tokens: 0 or 2 modulo 4): word k is the aligned word at a0 + 4 k, bytes outside Q read as 0
        const uintptr_t qbeg = (uintptr_t)Q, qend = (uintptr_t)(Q + m);
        const uintptr_t a0 = q0 & ~(uintptr_t)3;
        const int words = score_stage_words<Sym>(ge);
        for (int k = threadIdx.x; k < words; k += SCORE_THREADS) s_w[k] = match_aligned_word(a0 + 4 * (uintptr_t)k, qbeg, qend);
        if (threadIdx.x == 0) {
            int64_t next = m;
            s_doc[0] = q_off && tile0 < m ? score_doc_start(q_off, ndocs, m, tile0, &next) : 0;
            s_doc[1] = next;
        }
    }
    __syncthreads();
    const uint32_t sh0 = (uint32_t)(q0 & 3u) + SB * (uint32_t)ge;                 // the staged byte offset of Q[tile0]
    const int gl = (int)threadIdx.x & (G - 1), gi = (int)threadIdx.x / G, gshift = lane_id() & ~(G - 1);
    const uint32_t N1 = (uint32_t)n + 1u;
    unsigned long long symbols = 0, searches = 0, lookups = 0, zero = 0;
    for (int it = 0; it < SCORE_TILE / GROUPS; ++it) {
        const int64_t j = tile0 + (int64_t)it * GROUPS + gi;
        bool is_long = false;
        uint32_t lo = 0, hi = N1;
        if (j < m) {
            int64_t next;
            const int64_t start = j < s_doc[1] ? s_doc[0] : score_doc_start(q_off, ndocs, m, j, &next);
            const int64_t cap = j - start < max_len ? j - start : max_len;
            const int64_t limit = cap < (int64_t)ge ? cap : (int64_t)ge;
            const uint32_t at = sh0 + SB * (uint32_t)(j - tile0);                 // the staged byte offset of Q[j]
            int64_t good = 0, bad = cap + 1, step = 1;
            auto probe = [&](int64_t s) {
                const NgRange r = score_group_range<G>(T, SA, n, bkt, s_w, at - SB * (uint32_t)s, s, gl, gshift, &symbols);
                ++searches;
                if (r.hi > r.lo && r.hi - r.lo >= min_count) { good = s; lo = r.lo; hi = r.hi; } else bad = s;
            };
            while (good < limit && bad > cap) {
                probe(step < limit ? step : limit);
                step <<= 1;
            }
            if (bad > cap && cap > (int64_t)ge) {
                is_long = true;                                                   // ge symbols are good and the document has more
            } else {
                while (bad - good > 1) probe(good + (bad - good) / 2);
                const int sym = (int)(match_lds_word(s_w, at) & score_sym_mask<Sym>());
                uint32_t pr = 0;
                zero += score_finish(T, SA, n, j, good, lo, hi, sym, gshift, (gl & 1) != 0, out, &pr);
                if (gl < 2) lookups += pr;
            }
        }
        const int64_t slot = lcp_wave_append(is_long && gl == 0, (uint32_t *)&ctl[SC_W_LONG]);
        if (slot >= 0) { long_list[slot] = (uint32_t)j; long_lo[slot] = lo; long_hi[slot] = hi; }
    }
    if (gl != 0) { symbols = 0; searches = 0; }                   // (the lanes of a group count the same)
    lcp_block_add(symbols, &ctl[SC_W_BYTES]);
    lcp_block_add(searches, &ctl[SC_W_GROUP_SEARCHES]);
    lcp_block_add(lookups, &ctl[SC_W_LOOKUPS]);
    lcp_block_add(zero, &ctl[SC_W_ZERO]);
}

// One wave per entry of the long list: ge symbols are good with the range listed; the gallop goes on with the next power of two.
// bkt / pair / log_p: the byte index's tables, nullptr, nullptr, 0 for any other Sym (ngram_range).
template <typename Sym>
__global__ __launch_bounds__(SCORE_THREADS) void k_score_long(
    const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ bkt,
    const uint64_t *__restrict__ pair, int log_p, const Sym *__restrict__ Q, int64_t m, const int64_t *__restrict__ q_off, int64_t ndocs,
    uint32_t min_count, int64_t max_len, int ge, const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ long_lo,
    const uint32_t *__restrict__ long_hi, int64_t count, ScoreOut out, unsigned long long *__restrict__ ctl)
{
    const int64_t q = ((int64_t)blockIdx.x * SCORE_THREADS + threadIdx.x) / WAVE;
    if (q >= count) return;                                     // whole waves leave together
    const int64_t j = (int64_t)long_list[q];
    if (j >= m) return;
    int64_t next;
    const int64_t start = q_off ? score_doc_start(q_off, ndocs, m, j, &next) : 0;
    const int64_t cap = j - start < max_len ? j - start : max_len;
    int64_t good = (int64_t)ge < cap ? (int64_t)ge : cap, bad = cap + 1, step = 1, symbols = 0;
    unsigned long long searches = 0;
    uint32_t lo = long_lo[q], hi = long_hi[q];
    while (step <= good) step <<= 1;
    auto probe = [&](int64_t s) {
        const NgRange r = ngram_range(T, SA, n, bkt, pair, log_p, Q + (j - s), s, &symbols);
        ++searches;
        if (r.hi > r.lo && r.hi - r.lo >= min_count) { good = s; lo = r.lo; hi = r.hi; } else bad = s;
    };
    while (good < cap && bad > cap) {
        probe(step < cap ? step : cap);
        step <<= 1;
    }
    while (bad - good > 1) probe(good + (bad - good) / 2);
    uint32_t pr = 0;
    const uint32_t zero = score_finish(T, SA, n, j, good, lo, hi, (int)Q[j], 0, (lane_id() & 1) != 0, out, &pr);
    const uint32_t pr1 = (uint32_t)__shfl((int)pr, 1, WAVE);
    if (lane_id() != 0) return;
    atomicAdd(&ctl[SC_W_LONG_SEARCHES], searches);
    atomicAdd(&ctl[SC_W_LOOKUPS], (unsigned long long)pr + pr1);
    if (symbols) atomicAdd(&ctl[SC_W_BYTES], (unsigned long long)symbols);
    if (zero) atomicAdd(&ctl[SC_W_ZERO], 1ull);
}

}  // namespace sa
