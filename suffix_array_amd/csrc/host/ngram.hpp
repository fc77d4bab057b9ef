// host/ngram.hpp -- n-gram / infinity-gram queries over a device-resident index (kernels/ngram.hpp):
// sa_amd_index_next_bytes (the ranges by the search kernels, as host/docs.hpp gets them) and sa_amd_index_infgram (the ranges
// by the back-off kernel), then for both the continuations: count, one scan, ordered emission.
#pragma once
#include "docs.hpp"
#include "../kernels/ngram.hpp"

namespace sa {

static thread_local sa_amd_ngram_stats g_last_ngram_stats;
static thread_local int32_t g_ngram_stream_cap = -1;    // sa_amd_ngram_set_stream_cap of the calling thread (-1: NG_STREAM_CAP_DEFAULT)

// one wave per query, a wave takes every waves-th query: the counters cost one atomic per wave, not per query
static unsigned ngram_grid(int64_t queries)
{
    int64_t g = ceil_div(queries, NG_WAVES);
    const int64_t most = (int64_t)cu_count() * 16;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}

// backoff == false: sa_amd_index_next_bytes (suffix_len is nullptr).  backoff == true: sa_amd_index_infgram.  Host pointers,
// every output may be nullptr, arguments checked by the caller.  All scratch is one pooled block: 8 bytes per query for the
// listing (the continuations are computed twice -- counted, then emitted -- instead of kept at 1 KiB per query), and the
// device side of the listing, min(capacity, 256 count) entries.  One blocking read-back: the listing's length and the counters.
static int ngram_query(const sa_amd_index &ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, bool backoff, int32_t min_count,
                       int32_t max_len, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end, int64_t *list_off,
                       uint8_t *bytes, uint32_t *counts, int64_t capacity, int64_t *total_out)
{
    sa_amd_ngram_stats ns;
    memset(&ns, 0, sizeof(ns));
    ns.patterns = count;
    ns.stream_cap = g_ngram_stream_cap < 0 ? NG_STREAM_CAP_DEFAULT : g_ngram_stream_cap;
    ns.backoff = backoff ? 1 : 0;
    ns.compared_bytes = backoff ? 0 : -1;
    g_last_ngram_stats = ns;
    if (count == 0) {
        if (list_off) list_off[0] = 0;
        if (total_out) *total_out = 0;
        return SA_AMD_OK;
    }
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const int rb0 = g_readbacks;
    const size_t C = (size_t)count, total = (size_t)pat_off[count];
    const bool want = bytes || counts;
    const int64_t most = 256 * (int64_t)count;
    const size_t cap = want ? (size_t)(capacity < most ? capacity : most) : 0;

    PooledScope sc(ix.device, false);
    const size_t b_pat = align_up(total + 16, 256), b_off = align_up((C + 1) * 8, 256), b_w = align_up(C * 4 + 4, 256), b_b = align_up(C + 4, 256);
    const size_t b_ts = align_up(docs_scan_words((int64_t)C + 1) * 8, 256);
    const size_t b_lb = align_up(cap + 8, 256), b_lc = align_up(cap * 4 + 8, 256);
    sc.acquire(256 + b_pat + 2 * b_off + 3 * b_w + b_b + b_ts + b_lb + b_lc);
    unsigned long long *ctl = (unsigned long long *)sc.take(256);
    uint8_t *dP = (uint8_t *)sc.take(b_pat);
    int64_t *dO = (int64_t *)sc.take(b_off);
    unsigned long long *nnz = (unsigned long long *)sc.take(b_off), *tsum = (unsigned long long *)sc.take(b_ts);
    uint32_t *dLo = (uint32_t *)sc.take(b_w), *dHi = (uint32_t *)sc.take(b_w), *dLen = (uint32_t *)sc.take(b_w);
    uint8_t *dEnd = (uint8_t *)sc.take(b_b), *dBytes = (uint8_t *)sc.take(b_lb);
    uint32_t *dCounts = (uint32_t *)sc.take(b_lc);
    if (sc.rc) return sc.rc;
    hipStream_t st = sc.st;
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    HIP_TRY(hipMemsetAsync(nnz + C, 0, 8, st));
    if (total) HIP_TRY(hipMemcpyAsync(dP, pat_data, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dO, pat_off, (C + 1) * 8, hipMemcpyHostToDevice, st));

    // ---- the ranges: the search kernels as sa_amd_index_search runs them, or the back-off ----
    const unsigned grid = ngram_grid(count);
    if (backoff) {
        PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_infgram_suffix, dim3(grid), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n, ix.bkt(), ix.pair(),
                                                    esa_log_p(ix.n), (const uint8_t *)dP, (const int64_t *)dO, count, (uint32_t)min_count, (int64_t)max_len, dLen,
                                                    dLo, dHi, ctl));
    } else {
        g_prof.begin(KC_MISC, count, st);
        const int rcs = launch_search(ix.text(), ix.sa(), ix.n, ix.bkt(), ix.pair(), dP, dO, count, nullptr, dLo, dHi, nullptr, nullptr, nullptr, st);
        g_prof.end(st);
        if (rcs) return rcs;
    }
    // ---- the continuations: counted, scanned, emitted in order ----
    const uint32_t *depth = backoff ? dLen : nullptr;
    PROF(KC_MISC, count, st, hipLaunchKernelGGL((k_next_bytes<false>), dim3(grid), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                (const uint32_t *)dLo, (const uint32_t *)dHi, depth, (const int64_t *)dO, count, (uint32_t)ns.stream_cap, dEnd,
                                                nnz, (uint8_t *)nullptr, (uint32_t *)nullptr, 0ull, ctl));
    { const int rcn = docs_scan(nnz, (int64_t)count + 1, tsum, &ctl[NG_W_TOTAL], st); if (rcn) return rcn; }
    if (cap > 0)
        PROF(KC_MISC, count, st, hipLaunchKernelGGL((k_next_bytes<true>), dim3(grid), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                    (const uint32_t *)dLo, (const uint32_t *)dHi, depth, (const int64_t *)dO, count, (uint32_t)ns.stream_cap,
                                                    (uint8_t *)nullptr, nnz, bytes ? dBytes : (uint8_t *)nullptr, counts ? dCounts : (uint32_t *)nullptr,
                                                    (unsigned long long)cap, ctl));
    unsigned long long cw[NG_W_COUNT];
    { const int rcw = read_words(cw, ctl, sizeof(cw), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t listed = (int64_t)cw[NG_W_TOTAL];
    if (listed < 0 || listed > most) return SA_AMD_EINTERNAL;
    const size_t wr = (size_t)listed < cap ? (size_t)listed : cap;

    // ---- down: straight into the caller's arrays ----
    if (suffix_len) sc.down(suffix_len, dLen, C * 4);
    if (range_lo) sc.down(range_lo, dLo, C * 4);
    if (range_hi) sc.down(range_hi, dHi, C * 4);
    if (at_end) sc.down(at_end, dEnd, C);
    if (bytes && wr > 0) sc.down(bytes, dBytes, wr);
    if (counts && wr > 0) sc.down(counts, dCounts, wr * 4);
    if (list_off) sc.down(list_off, nnz, (C + 1) * 8);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    if (total_out) *total_out = listed;
    g_prof.resolve();
    ns.range_searches = backoff ? (int64_t)cw[NG_W_SEARCHES] : (int64_t)count;
    if (backoff) ns.compared_bytes = (int64_t)cw[NG_W_BYTES];
    ns.stream_slots = (int64_t)cw[NG_W_STREAM_SLOTS];
    ns.search_slots = (int64_t)cw[NG_W_SEARCH_SLOTS];
    ns.stream_queries = (int64_t)cw[NG_W_STREAM_Q];
    ns.search_queries = (int64_t)cw[NG_W_SEARCH_Q];
    ns.empty_queries = (int64_t)cw[NG_W_EMPTY_Q];
    ns.entries = listed;
    ns.passes = cap > 0 ? 2 : 1;
    ns.readbacks = g_readbacks - rb0;
    g_last_ngram_stats = ns;
    return SA_AMD_OK;
}

}  // namespace sa
