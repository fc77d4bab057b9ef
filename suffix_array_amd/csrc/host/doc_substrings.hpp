// host/doc_substrings.hpp -- repeated substrings with their document frequency over a device-resident index with a collection
// (kernels/doc_substrings.hpp): work-block layout, the document table's stage inside substrings_run and
// the host-pointer route of sa_amd_index_doc_substrings.
//
// Buffers.  The work block is that of host/substrings.hpp | GE (n + 2 entries, rounded as the n-entry buffers are).  What
// host/substrings.hpp says of its part holds here; what this route adds:
//   stage 1       as there: psl in A0, nsl in A1, the levels of minima in A2.
//   pair pass     G in GE, cleared first; the range-minimum queries read LCPV and the levels in A2, which therefore still stand:
//                 the pass runs behind lz_nsv<true> and before the ranked node pass puts the candidates' keys over A2 | A3.
//   scan          GE in place, G -> E; the tiles' sums in the LCP block's tile words, which the node pass takes over afterwards.
//   node pass     reads E[hi] and E[lo + 1] beside LCPV, psl and nsl; ORDER_ALL writes df beside the rows.
//   gather        reads E again for the df of the rows it writes.  GE stays to the end.
// Control words: the DSUB_C_* words lie at byte 64 of the LCP control slab, over the LCP build's own words, which are dead once
// its front end has been read back; they are cleared in front of the pair pass.
// Read-backs, all through read_words and counted: those of host/substrings.hpp, not one more -- the table's counters come back
// with the node pass's.
#pragma once
#include "substrings.hpp"
#include "docs.hpp"
#include "../kernels/doc_substrings.hpp"

namespace sa {

static thread_local sa_amd_doc_substr_stats g_last_doc_substr_stats;
#ifdef SA_AMD_DIAG
// the pair pass without the combining of equal targets inside a wave, in the diagnostic library only
// (sa_amd_debug_dsub_plain_atomics) -- for the A/B of tools/doc_substrings_bench.py; the table is the same
inline std::atomic<int> g_dsub_plain_atomics{0};
#endif

constexpr int DSUB_CTL_OFF = LCP_CTL_OFF;   // byte offset of the DSUB_C_* words in the LCP control slab
constexpr int DSUB_C_GSUM = DSUB_C_WORDS;   // the scan's total, one word behind the kernels' own
static_assert(DSUB_CTL_OFF + (DSUB_C_GSUM + 1) * 8 <= SUB_CTL_OFF, "control slab");
static_assert(SA_AMD_SUBSTR_BY_DOCS == SUB_ORDER_DOCS, "the kernels take the ABI's order");

struct DsubLayout { SubLayout sub; size_t ge, bytes; };
static DsubLayout dsub_layout(int32_t n)
{
    DsubLayout D;
    D.sub = sub_layout(n);
    D.ge = D.sub.bytes;
    D.bytes = D.ge + align_up(D.sub.lcp.alt_elems * 4, 256);
    return D;
}

// what needs no device: the query's ranges and the output arguments
static bool dsub_args_ok(const sa_amd_doc_substr_query *q, const uint32_t *rows, int64_t capacity, const int64_t *total)
{
    if (!q || !total || capacity < 0 || (capacity > 0 && !rows)) return false;
    if (q->min_len < 1 || q->max_len < 0 || (q->max_len != 0 && q->max_len < q->min_len) || q->min_count < 2 || q->min_docs < 1) return false;
    if (q->order < SA_AMD_SUBSTR_ALL || q->order > SA_AMD_SUBSTR_BY_DOCS) return false;
    return q->order == SA_AMD_SUBSTR_ALL || q->k >= 1;
}

// The Docs of substrings_run for an index with a collection: builds E, hands it to the node pass and the gather, reads the counters.
struct SubDocTable {
    static constexpr bool on = true;
    const uint32_t *prev;                   // the collection's per-slot word, n + 1 entries
    uint32_t min_docs;
    uint32_t *dDf;                          // the df column beside dRows, or null
    const DsubLayout &D;
    sa_amd_doc_substr_stats &ds;
    uint32_t *E = nullptr;
    unsigned long long *dctl = nullptr;

    // lcpv: LCP[0 .. N1) in slot order; lv: its levels of minima, still standing; base: the work block
    int table(const uint32_t *lcpv, int64_t N1, const LzLevels &lv, char *base, hipStream_t st)
    {
        const LcpLayout &L = D.sub.lcp;
        E = (uint32_t *)(base + D.ge);
        dctl = (unsigned long long *)(base + L.ctl + DSUB_CTL_OFF);
        const int64_t len = N1 + 1;
        HIP_TRY(hipMemsetAsync(dctl, 0, (DSUB_C_GSUM + 1) * 8, st));
        HIP_TRY(hipMemsetAsync(E, 0, (size_t)len * 4, st));
        int64_t pgs = ceil_div(N1, LZ_THREADS);
        const int64_t most = (int64_t)cu_count() * 32;              // resident workgroups that walk over the slots
        const unsigned pg = (unsigned)(pgs < most ? pgs : most);
        bool combine = true;
#ifdef SA_AMD_DIAG
        combine = g_dsub_plain_atomics.load() == 0;
#endif
        if (combine) PROF(KC_REP_SPANS, N1, st, hipLaunchKernelGGL((k_dsub_pairs<true>), dim3(pg), dim3(LZ_THREADS), 0, st, lcpv, N1, prev, lv, E, dctl));
        else PROF(KC_REP_SPANS, N1, st, hipLaunchKernelGGL((k_dsub_pairs<false>), dim3(pg), dim3(LZ_THREADS), 0, st, lcpv, N1, prev, lv, E, dctl));
        uint32_t *cnt = (uint32_t *)(base + L.tiles);
        const int64_t tiles = ceil_div(len, REP_TILE);
        PROF(KC_REP_SPANS, len, st, hipLaunchKernelGGL((k_dsub_scan<0>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, E, len, cnt));
        PROF(KC_REP_SPANS, tiles, st, hipLaunchKernelGGL(k_rep_sum_spine, dim3(1), dim3(REP_SPINE_THREADS), 0, st, cnt, tiles, &dctl[DSUB_C_GSUM]));
        PROF(KC_REP_SPANS, len, st, hipLaunchKernelGGL((k_dsub_scan<1>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, E, len, cnt));
        return SA_AMD_OK;
    }
    SubDf df() const { return SubDf{ E, min_docs, dDf, dctl }; }
    // head: the first 256 bytes of the control slab as the node pass's read-back brought them
    void counters(const uint32_t *head)
    {
        unsigned long long cw[DSUB_C_GSUM + 1];
        memcpy(cw, (const char *)head + DSUB_CTL_OFF, sizeof(cw));
        ds.df_sum = (int64_t)cw[DSUB_C_DFSUM];
        ds.max_df = (int64_t)cw[DSUB_C_MAXDF];
        ds.pairs = (int64_t)cw[DSUB_C_PAIRS];
        ds.rmq_far = (int64_t)cw[DSUB_C_FAR];
        ds.rmq_steps = (int64_t)cw[DSUB_C_STEPS];
        ds.rmq_max = (int64_t)cw[DSUB_C_RMAX];
    }
};
static_assert(REP_TILE == LCP_TILE, "the scan's tile sums live in the LCP block's tile words");

// the index's resident text, array and collection: the work block and the three output slabs come from the pool; on the null
// stream.  The convention of substrings_resident: min(count, cap) rows come down, *total is written only behind a successful wait.
static int32_t doc_substrings_index(const sa_amd_index &ix, const sa_amd_doc_substr_query *q, uint32_t *rows, uint32_t *df, uint32_t *pos,
                                    int64_t capacity, int64_t *total)
{
    if (!dsub_args_ok(q, rows, capacity, total) || !ix.doc_prev()) return SA_AMD_EINVAL;
    sa_amd_doc_substr_stats ds;
    memset(&ds, 0, sizeof(ds));
    g_last_doc_substr_stats = ds;
    const sa_amd_substr_query Q = { q->min_len, q->max_len, q->min_count, q->order, q->k };
    const int64_t cap = sub_row_cap(ix.n, Q, capacity);
    const DsubLayout D = dsub_layout(ix.n);
    PooledScope sc(ix.device, false);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), D.bytes, align_up(sub_rows_bytes(cap), 256) + 2 * align_up(sub_pos_bytes(cap), 256));
    uint32_t *dRows = (uint32_t *)sc.take(sub_rows_bytes(cap)), *dPos = (uint32_t *)sc.take(sub_pos_bytes(cap));
    uint32_t *dDf = (uint32_t *)sc.take(sub_pos_bytes(cap));
    int64_t count = 0;
    sa_amd_substr_stats ss;
    memset(&ss, 0, sizeof(ss));
    if (sc.rc == SA_AMD_OK) {
        const uint32_t min_docs = q->min_docs > (int64_t)0xffffffff ? 0xffffffffu : (uint32_t)q->min_docs;      // (df < 2^31: nothing passes either)
        SubDocTable docs{ ix.doc_prev(), min_docs, df ? dDf : nullptr, D, ds };
        sc.rc = substrings_run(in.dT, in.dSA, ix.n, Q, dRows, pos ? dPos : nullptr, cap, &count, in.dW, D.sub, sc.st, ss, docs);
    }
    const int64_t wr = count < cap ? count : cap;
    if (wr > 0) sc.down(rows, dRows, (size_t)wr * 16);
    if (wr > 0 && df) sc.down(df, dDf, (size_t)wr * 4);
    if (wr > 0 && pos) sc.down(pos, dPos, (size_t)wr * 4);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    *total = count;
    ds.nodes = ss.nodes;
    ds.selected = ss.selected;
    ds.distinct_selected = ss.distinct_selected;
    ds.sorted = ss.sorted;
    ds.select_passes = ss.select_passes;
    ds.readbacks = ss.readbacks;
    g_last_doc_substr_stats = ds;
    return SA_AMD_OK;
}

}  // namespace sa
