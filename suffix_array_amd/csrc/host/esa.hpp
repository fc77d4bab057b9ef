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

// sa_amd_index_search behind its argument checks: the patterns go up in buffers of the call's own, the outputs (each may be
// nullptr) come back by blocking copies; the thread's search statistics are those of this call
static int32_t index_search(const sa_amd_index &ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, uint8_t *contains,
                            uint32_t *range_lo, uint32_t *range_hi, uint32_t *lcp_start, uint32_t *lcp_len)
{
    if (count == 0) {
        sa_amd_search_stats z;
        memset(&z, 0, sizeof(z));
        z.route = ix.pair() ? 1 : 0;
        if (!ix.pair()) z.compared_bytes = z.steps = z.table_steps = -1;
        g_last_search_stats = z;
        return SA_AMD_OK;
    }
    const int64_t total = pat_off[count];
    DeviceGuard guard(ix.device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    const size_t C = (size_t)count;
    DevBuf dP, dO, dC, dR;
    int32_t rc;
    if ((rc = dP.alloc((size_t)total))) return rc;
    if ((rc = dO.alloc((C + 1) * 8))) return rc;
    if ((rc = dC.alloc(C))) return rc;
    if ((rc = dR.alloc(C * 4 * 4))) return rc;
    if (total) HIP_TRY(hipMemcpy(dP.p, pat_data, (size_t)total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dO.p, pat_off, (C + 1) * 8, hipMemcpyHostToDevice));
    uint32_t *R = dR.as<uint32_t>();
    sa_amd_search_stats stats;
    memset(&stats, 0, sizeof(stats));
    stats.patterns = count;
    stats.compared_bytes = stats.steps = stats.table_steps = -1;
    DevBuf dS;
    if (ix.pair()) {                                             // LCP route (kernels/esa.hpp): its three counters
        if ((rc = dS.alloc(3 * 8))) return rc;
        HIP_TRY(hipMemset(dS.p, 0, 3 * 8));
    }
    if ((rc = launch_search(ix.text(), ix.sa(), ix.n, ix.bkt(), ix.pair(), dP.as<const uint8_t>(), dO.as<const int64_t>(), count, dC.as<uint8_t>(), R, R + C,
                            R + 2 * C, R + 3 * C, ix.pair() ? dS.as<unsigned long long>() : nullptr, nullptr))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (ix.pair()) {
        int64_t cw[3];
        HIP_TRY(hipMemcpy(cw, dS.p, sizeof(cw), hipMemcpyDeviceToHost));
        stats.compared_bytes = cw[0]; stats.steps = cw[1]; stats.table_steps = cw[2];
        stats.route = 1;
    }
    g_last_search_stats = stats;
    if (contains) HIP_TRY(hipMemcpy(contains, dC.p, C, hipMemcpyDeviceToHost));
    if (range_lo) HIP_TRY(hipMemcpy(range_lo, R, C * 4, hipMemcpyDeviceToHost));
    if (range_hi) HIP_TRY(hipMemcpy(range_hi, R + C, C * 4, hipMemcpyDeviceToHost));
    if (lcp_start) HIP_TRY(hipMemcpy(lcp_start, R + 2 * C, C * 4, hipMemcpyDeviceToHost));
    if (lcp_len) HIP_TRY(hipMemcpy(lcp_len, R + 3 * C, C * 4, hipMemcpyDeviceToHost));
    return SA_AMD_OK;
}

// sa_amd_index_enable_lcp: the pair table, built once from the LCP array and kept
static int32_t index_enable_lcp(sa_amd_index &ix)
{
    if (ix.pair()) return SA_AMD_OK;
    PooledScope sc(ix.device, false);
    if (sc.rc) return sc.rc;
    DevBuf pair;
    if (index_table_alloc(pair, ((size_t)ix.n + 1) * 8) != SA_AMD_OK) return SA_AMD_ENOMEM;
    // LCP array and its work block from the pool, as sa_amd_index_lcp; the tile minima of the table build behind them
    const size_t lb = align_up(((size_t)ix.n + 1) * 4, 256), mb = esa_mins_elems(ix.n) * 4;
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), lcp_layout(ix.n).bytes, lb + mb);
    uint32_t *dL = (uint32_t *)sc.take(lb), *dMins = (uint32_t *)sc.take(mb);
    if (sc.rc == SA_AMD_OK) sc.rc = lcp_device(in.dT, in.dSA, ix.n, dL, in.dW, (int64_t)in.wb, sc.st);
    if (sc.rc == SA_AMD_OK) sc.rc = esa_build(dL, ix.n, pair.as<uint64_t>(), dMins, sc.st);
    if (sc.rc == SA_AMD_OK) sc.rc = hip_status(hipDeviceSynchronize());      // (the route's own wait: finish() adds none on success)
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    ix.dPair = std::move(pair);                                 // kept: later searches take the LCP route
    return SA_AMD_OK;
}

}  // namespace sa
