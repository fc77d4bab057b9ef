// host/doc_match.hpp -- Boolean document queries over a device-resident index (kernels/doc_match.hpp):
// the ranges and units of all patterns by docs_ranges, then slab by slab the clauses' bitmaps (zeroed, marked) and the queries'
// AND / NOT over them; document frequencies, or the listing in ascending document id.
#pragma once
#include "docs.hpp"
#include "../kernels/doc_match.hpp"

namespace sa {

constexpr int64_t DM_BUDGET_DEFAULT = (int64_t)256 << 20, DM_BUDGET_MIN = 4096, DM_BUDGET_MAX = (int64_t)1 << 40;
static thread_local sa_amd_doc_match_stats g_last_doc_match_stats;
static thread_local int64_t g_dm_budget = -1;           // sa_amd_doc_match_set_budget of the calling thread (-1: DM_BUDGET_DEFAULT)

// off[0 .. count]: starts at 0, never decreases, ends at `last`
static bool dm_offsets_valid(const int32_t *off, int32_t count, int32_t last)
{
    if (count < 0 || !off || off[0] != 0 || off[count] != last) return false;
    for (int32_t i = 0; i < count; ++i) if (off[i + 1] < off[i]) return false;
    return true;
}

// everything about the arguments that can be checked without the index
static bool doc_match_args_valid(const uint8_t *pat_data, const int64_t *pat_off, int32_t npat, const int32_t *clause_off, const uint8_t *clause_flags,
                                 int32_t nclauses, const int32_t *query_off, int32_t nqueries)
{
    if (!search_patterns_valid(pat_data, pat_off, npat)) return false;
    if (!dm_offsets_valid(clause_off, nclauses, npat) || !dm_offsets_valid(query_off, nqueries, nclauses)) return false;
    if (clause_flags) for (int32_t c = 0; c < nclauses; ++c) if (clause_flags[c] & ~1u) return false;
    return true;
}

// Consecutive whole queries form a slab while their clauses' bitmaps (4 W bytes each) fit the budget; a slab holds at least one
// query, so a query that alone exceeds the budget is a slab of its own.  -> the first query of every slab, and nqueries.
static std::vector<int32_t> dm_slabs(const int32_t *query_off, int32_t nqueries, int64_t W, int64_t budget)
{
    std::vector<int32_t> first;
    for (int32_t q = 0; q < nqueries;) {
        first.push_back(q);
        int64_t rows = (int64_t)query_off[q + 1] - query_off[q];
        for (++q; q < nqueries; ++q) {
            const int64_t more = (int64_t)query_off[q + 1] - query_off[q];
            if ((rows + more) * 4 * W > budget) break;
            rows += more;
        }
    }
    first.push_back(nqueries);
    return first;
}

static unsigned dm_item_grid(int64_t items)
{
    int64_t g = ceil_div(items, DM_THREADS / WAVE);
    const int64_t most = (int64_t)cu_count() * 32;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}

// !list: df (nqueries entries) and clause_df (nclauses entries), either may be nullptr.  list: list_off (nqueries + 1 entries), the
// first `capacity` documents to docs, the number of all of them to *total_out.  Host pointers, arguments checked by the caller.
template <typename Index>
static int doc_match_query(const Index &ix, const typename DocsSym<Index>::type *pat_data, const int64_t *pat_off, int32_t npat, const int32_t *clause_off,
                           const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off, int32_t nqueries, bool list, uint32_t *df_out,
                           uint32_t *cdf_out, int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    const uint32_t ndocs = ix.ndocs;
    const uint32_t W = (uint32_t)(((uint64_t)ndocs + 31) / 32), stride = (W + DM_LANE_WORDS - 1) / DM_LANE_WORDS * DM_LANE_WORDS;
    const uint32_t tiles = (uint32_t)ceil_div((int64_t)W, DM_TILE_WORDS);
    sa_amd_doc_match_stats ms;
    memset(&ms, 0, sizeof(ms));
    ms.patterns = npat; ms.clauses = nclauses; ms.queries = nqueries;
    ms.bitmap_words = W;
    ms.budget = g_dm_budget < 0 ? DM_BUDGET_DEFAULT : g_dm_budget;
    ms.chunk = (int32_t)(g_docs_chunk < 0 ? DOC_CHUNK_DEFAULT : g_docs_chunk);
    ms.listed = list ? 1 : 0;
    g_last_doc_match_stats = ms;
    if (nqueries == 0) {
        if (list) { list_off[0] = 0; *total_out = 0; }
        return SA_AMD_OK;
    }
    const size_t P = (size_t)npat, C = (size_t)nclauses, Q = (size_t)nqueries;
    const std::vector<int32_t> slab = dm_slabs(query_off, nqueries, W, ms.budget);
    const size_t nslabs = slab.size() - 1;
    ms.slabs = (int64_t)nslabs;
    size_t max_rows = 0;
    for (size_t s = 0; s < nslabs; ++s) {
        const size_t rows = (size_t)(query_off[slab[s + 1]] - query_off[slab[s]]);
        max_rows = rows > max_rows ? rows : max_rows;
    }
    std::vector<uint32_t> pcl(P + 1, 0u);                     // pattern -> clause
    for (size_t c = 0; c < C; ++c) for (int32_t p = clause_off[c]; p < clause_off[c + 1]; ++p) pcl[(size_t)p] = (uint32_t)c;
    std::vector<uint8_t> flags(C + 1, (uint8_t)0);
    if (clause_flags && C) memcpy(flags.data(), clause_flags, C);

    const int rb0 = g_readbacks;
    DocsBatch b(ix.device);
    if (b.sc.rc) return b.sc.rc;
    if (npat > 0) { const int rcr = docs_ranges(b, ix, pat_data, pat_off, npat, false); if (rcr) return rcr; }
    hipStream_t st = b.sc.st;
    ms.occ_sum = (int64_t)b.occ_sum;
    ms.units = (int64_t)b.units;
    if (npat == 0) b.chunk = (uint32_t)ms.chunk;

    // ---- the call's block: the query's shape, the outputs, the listing's scan, one slab of bitmaps ----
    const size_t items = Q * tiles;
    const int64_t bound = (int64_t)Q * (int64_t)ndocs;
    const int64_t cap = capacity < bound ? capacity : bound;
    const size_t b_pcl = align_up(P * 4 + 4, 256), b_fl = align_up(C + 4, 256), b_qo = align_up((Q + 1) * 4, 256), b_df = align_up(Q * 4 + 4, 256);
    const size_t b_cdf = align_up(C * 4 + 4, 256), b_tc = list ? align_up((items + 1) * 8, 256) : 0;
    const size_t b_ts = list ? align_up(docs_scan_words((int64_t)items + 1) * 8, 256) : 0, b_lo = list ? align_up((Q + 1) * 8, 256) : 0;
    const size_t b_docs = list ? align_up((size_t)cap * 4 + 8, 256) : 0, b_bits = align_up(max_rows * stride * 4 + 4, 256);
    PooledScope s2(-1, false);
    s2.acquire(256 + b_pcl + b_fl + b_qo + b_df + b_cdf + b_tc + b_ts + b_lo + b_docs + b_bits);
    unsigned long long *ctl = (unsigned long long *)s2.take(256);
    uint32_t *dPcl = (uint32_t *)s2.take(b_pcl);
    uint8_t *dFl = (uint8_t *)s2.take(b_fl);
    int32_t *dQo = (int32_t *)s2.take(b_qo);
    uint32_t *dDf = (uint32_t *)s2.take(b_df), *dCdf = (uint32_t *)s2.take(b_cdf);
    unsigned long long *tcnt = list ? (unsigned long long *)s2.take(b_tc) : nullptr, *tsum = list ? (unsigned long long *)s2.take(b_ts) : nullptr;
    long long *dLoff = list ? (long long *)s2.take(b_lo) : nullptr;
    uint32_t *dDocs = list ? (uint32_t *)s2.take(b_docs) : nullptr;
    uint32_t *bits = (uint32_t *)s2.take(b_bits);
    if (s2.rc) return s2.rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    HIP_TRY(hipMemsetAsync(dDf, 0, Q * 4, st));
    if (C) HIP_TRY(hipMemsetAsync(dCdf, 0, C * 4, st));
    if (P) HIP_TRY(hipMemcpyAsync(dPcl, pcl.data(), P * 4, hipMemcpyHostToDevice, st));
    if (C) HIP_TRY(hipMemcpyAsync(dFl, flags.data(), C, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dQo, query_off, (Q + 1) * 4, hipMemcpyHostToDevice, st));
    if (list) HIP_TRY(hipMemsetAsync(tcnt + items, 0, 8, st));

    // One slab: its bitmaps zeroed (a recycled block holds arbitrary bytes) and marked, then `emit` ? the listing's entries :
    // the counts.  The slabs follow one another on the stream: nothing comes back between them.
    const bool cdf = !list && cdf_out != nullptr;
    const uint32_t sstride = (uint32_t)ceil_div((int64_t)ndocs + 1, DOC_SAMPLES), ns = (uint32_t)ceil_div((int64_t)ndocs + 1, sstride);      // (as launch_doc_of)
    auto run_slab = [&](size_t s, bool emit, bool count_marks) -> int {
        const uint32_t q0 = (uint32_t)slab[s], q1 = (uint32_t)slab[s + 1];
        const uint32_t c0 = (uint32_t)query_off[q0], c1 = (uint32_t)query_off[q1];
        const uint32_t p0 = (uint32_t)clause_off[c0], p1 = (uint32_t)clause_off[c1];
        if (c1 > c0) HIP_TRY(hipMemsetAsync(bits, 0, (size_t)(c1 - c0) * stride * 4, st));
        if (b.units && p1 > p0)
            PROF(KC_MISC, (int64_t)b.occ_sum, st, hipLaunchKernelGGL(k_dm_mark, dim3(docs_unit_grid((int64_t)b.units)), dim3(DM_THREADS), 0, st, ix.doc_prev(),
                                                                     ix.sa(), (const uint32_t *)b.dLo, (const uint32_t *)b.dOcc,
                                                                     (const unsigned long long *)b.uoff, (const uint32_t *)dPcl, npat, b.units, p0, p1, c0, c1,
                                                                     b.chunk, ix.doc_off(), ndocs + 1u, sstride, ns, (uint32_t)ix.n, stride, bits,
                                                                     count_marks ? ctl : (unsigned long long *)nullptr));
        const int64_t its = (int64_t)(q1 - q0) * tiles;
        const dim3 grid(dm_item_grid(its)), block(DM_THREADS);
        if (emit)
            PROF(KC_MISC, its, st, hipLaunchKernelGGL(k_dm_emit, grid, block, 0, st, (const uint32_t *)bits, (const int32_t *)dQo, (const uint8_t *)dFl, q0, q1,
                                                      c0, c1, stride, W, ndocs, tiles, (const unsigned long long *)tcnt, dDocs, (unsigned long long)cap));
        else if (list)
            PROF(KC_MISC, its, st, hipLaunchKernelGGL((k_dm_combine<true, false>), grid, block, 0, st, (const uint32_t *)bits, (const int32_t *)dQo,
                                                      (const uint8_t *)dFl, q0, q1, c0, c1, stride, W, ndocs, tiles, dDf, dCdf, tcnt));
        else if (cdf)
            PROF(KC_MISC, its, st, hipLaunchKernelGGL((k_dm_combine<false, true>), grid, block, 0, st, (const uint32_t *)bits, (const int32_t *)dQo,
                                                      (const uint8_t *)dFl, q0, q1, c0, c1, stride, W, ndocs, tiles, dDf, dCdf, tcnt));
        else
            PROF(KC_MISC, its, st, hipLaunchKernelGGL((k_dm_combine<false, false>), grid, block, 0, st, (const uint32_t *)bits, (const int32_t *)dQo,
                                                      (const uint8_t *)dFl, q0, q1, c0, c1, stride, W, ndocs, tiles, dDf, dCdf, tcnt));
        return SA_AMD_OK;
    };
    for (size_t s = 0; s < nslabs; ++s) { const int rcs = run_slab(s, false, true); if (rcs) return rcs; }

    unsigned long long marks = 0;
    if (!list) {
        std::vector<uint32_t> df(Q), cdfv(cdf ? C : 0);
        HIP_TRY(hipStreamSynchronize(st));
        s2.down(df.data(), dDf, Q * 4);
        if (cdf && C) s2.down(cdfv.data(), dCdf, C * 4);
        s2.down(&marks, ctl, 8);
        if (s2.finish() != SA_AMD_OK) return s2.rc;
        if (b.sc.finish() != SA_AMD_OK) return b.sc.rc;          // the last step that can fail: nothing is written before it
        for (size_t q = 0; q < Q; ++q) ms.df_sum += df[q];
        if (df_out) memcpy(df_out, df.data(), Q * 4);
        if (cdf && C) memcpy(cdf_out, cdfv.data(), C * 4);
    } else {
        // one scan over the (query, tile) counts of all slabs: every tile's offset, and list_off[q] at the query's first tile
        { const int rcn = docs_scan(tcnt, (int64_t)items + 1, tsum, nullptr, st); if (rcn) return rcn; }
        PROF(KC_MISC, nqueries, st, hipLaunchKernelGGL(k_dm_list_off, dim3((unsigned)ceil_div((int64_t)nqueries + 1, DM_THREADS)), dim3(DM_THREADS), 0, st,
                                                       (const unsigned long long *)tcnt, tiles, nqueries, dLoff));
        if (cap > 0) {
            // the one slab's bitmaps are still there; those of several slabs were overwritten in turn and are marked again
            if (nslabs == 1) {
                const uint32_t c0 = 0, c1 = (uint32_t)nclauses;
                PROF(KC_MISC, (int64_t)items, st, hipLaunchKernelGGL(k_dm_emit, dim3(dm_item_grid((int64_t)items)), dim3(DM_THREADS), 0, st, (const uint32_t *)bits,
                                                                     (const int32_t *)dQo, (const uint8_t *)dFl, 0u, (uint32_t)nqueries, c0, c1, stride, W, ndocs,
                                                                     tiles, (const unsigned long long *)tcnt, dDocs, (unsigned long long)cap));
            } else {
                for (size_t s = 0; s < nslabs; ++s) { const int rcs = run_slab(s, true, false); if (rcs) return rcs; }
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<int64_t> loff(Q + 1);
        s2.down(loff.data(), dLoff, (Q + 1) * 8);
        s2.down(&marks, ctl, 8);
        if (s2.rc) return s2.rc;
        const int64_t listed = loff[Q];
        if (listed < 0 || listed > bound) return SA_AMD_EINTERNAL;
        const int64_t wr = listed < cap ? listed : cap;
        if (s2.finish() != SA_AMD_OK) return s2.rc;
        if (b.sc.finish() != SA_AMD_OK) return b.sc.rc;
        if (wr > 0) HIP_TRY(hipMemcpy(docs, dDocs, (size_t)wr * 4, hipMemcpyDeviceToHost));      // the last step that can fail; list_off and the total behind it
        memcpy(list_off, loff.data(), (Q + 1) * 8);
        *total_out = listed;
        ms.df_sum = listed;
    }
    g_prof.resolve();
    ms.marks = (int64_t)marks;
    ms.readbacks = g_readbacks - rb0;
    g_last_doc_match_stats = ms;
    return SA_AMD_OK;
}

}  // namespace sa
