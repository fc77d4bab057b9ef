// host/esa.hpp -- enhanced suffix array of a device-resident index (kernels/esa.hpp): the pair table's
// build from the LCP array and the launch of the LCP-accelerated search.
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

}  // namespace sa
