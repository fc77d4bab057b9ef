// host/esa.hpp -- enhanced suffix array of a device-resident index (kernels/esa.hpp): the pair table's
// build from the LCP array, and the launch of the batched search (plain or LCP-accelerated) that every index route shares.
#pragma once
#include "lcp.hpp"
#include "../kernels/esa.hpp"

namespace sa {

static thread_local sa_amd_search_stats g_last_search_stats;

// log2 P: P is the smallest power of two >= N + 1, N = n + 1 slots
static inline int esa_log_p(int32_t n)
{
    const uint64_t N = (uint64_t)n + 1;
    int k = 1;
    while ((1ull << k) < N + 1) ++k;
    return k;
}

// uint32 entries of tile minima esa_build passes between its launches
static inline size_t esa_mins_elems(int32_t n)
{
    const int64_t N = (int64_t)n + 1;
    return (size_t)((N >> ESA_TILE_LOG) + 1 + (N >> (2 * ESA_TILE_LOG)) + 1);
}

// dLCP: n + 1 entries; dPair: n + 1 pairs; dMins: esa_mins_elems(n) entries.  One launch per 12 levels of the tree (at most
// three); the tile minima of one launch are the input of the next.  Does not synchronise.
static int esa_build(const uint32_t *dLCP, int32_t n, uint64_t *dPair, uint32_t *dMins, hipStream_t st)
{
    const int64_t N = (int64_t)n + 1;
    const uint32_t *src = dLCP;
    int64_t src_len = N;
    uint32_t *mins = dMins;
    for (int shift = 0; (N >> shift) >= 1; shift += ESA_TILE_LOG) {
        const int64_t tiles = ((N >> shift) >> ESA_TILE_LOG) + 1;
        const bool last = (N >> (shift + ESA_TILE_LOG)) < 1;
        hipLaunchKernelGGL(k_esa_tree, dim3((unsigned)tiles), dim3(ESA_THREADS), 0, st, src, src_len, shift, N, dPair,
                           last ? (uint32_t *)nullptr : mins);
        LAUNCH_CHECK(st);
        src = mins; src_len = tiles;
        mins += tiles;
    }
    return SA_AMD_OK;
}

// the pattern arguments of the batched searches: count >= 0, pat_off[0 .. count] non-negative and non-decreasing, pattern bytes
// where there are any
static bool search_patterns_valid(const uint8_t *pat_data, const int64_t *pat_off, int32_t count)
{
    if (count < 0 || (count > 0 && !pat_off)) return false;
    if (count == 0) return true;
    const int64_t total = pat_off[count];
    if (total < 0 || (total > 0 && !pat_data)) return false;
    for (int32_t i = 0; i < count; ++i) if (pat_off[i + 1] < pat_off[i] || pat_off[i] < 0) return false;
    return true;
}

// The batched search of `count` > 0 uploaded patterns, one wave each: over the pair table when the index has one (dPair), else
// the plain binary search; dBkt narrows either (nullptr: no bucket table).  Every output may be nullptr; stats: the LCP route's
// three counters or nullptr.  Does not synchronise.
static int launch_search(const uint8_t *dT, const uint32_t *dSA, int32_t n, const uint32_t *dBkt, const uint64_t *dPair, const uint8_t *dP,
                         const int64_t *dO, int32_t count, uint8_t *contains, uint32_t *lo, uint32_t *hi, uint32_t *lcp_start, uint32_t *lcp_len,
                         unsigned long long *stats, hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div((int64_t)count * WAVE, SEARCH_THREADS));
    if (dPair)
        hipLaunchKernelGGL(k_esa_search, grid, dim3(SEARCH_THREADS), 0, st, dT, dSA, (int64_t)n, dPair, esa_log_p(n), dP, dO, count, contains, lo, hi,
                           lcp_start, lcp_len, dBkt, stats);
    else
        hipLaunchKernelGGL(k_search_batch, grid, dim3(SEARCH_THREADS), 0, st, dT, dSA, (int64_t)n, dP, dO, count, contains, lo, hi, lcp_start, lcp_len,
                           dBkt);
    LAUNCH_CHECK(st);
    return SA_AMD_OK;
}

}  // namespace sa
