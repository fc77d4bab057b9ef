// host/doc_repeats.hpp -- document-aware duplicate spans over a device-resident index (kernels/doc_repeats.hpp, DESIGN.md
// section 17): work-block layout, the device sequence and the host-pointer route of sa_amd_index_doc_repeat_spans.
#pragma once
#include "repeats.hpp"
#include "docs.hpp"
#include "../kernels/doc_repeats.hpp"

namespace sa {

static thread_local sa_amd_doc_repeat_stats g_last_doc_repeat_stats;

constexpr int DOCREP_CTL_OFF = REP_CTL_OFF + REP_C_WORDS * 8;        // byte offset of the DOCREP_C_* words in the LCP control slab
static_assert(DOCREP_CTL_OFF + DOCREP_C_WORDS * 8 <= 256, "control slab");

// layout of the work block: the repeat finder's block (whose n-entry buffer holds the flag bytes) | doc_bytes (ndocs words).
// After the front end the LCP block's four n-entry buffers hold: LCP in slot order | ds in slot order | de in slot order | the
// tiles' words (DOCREP_AGG of the slot pass, DOCREP_CARRY of the spine, one span count).
struct DocRepLayout { RepLayout rep; size_t doc_bytes, bytes; };
static DocRepLayout docrep_layout(int32_t n, int64_t ndocs)
{
    DocRepLayout D;
    D.rep = rep_layout(n);
    D.doc_bytes = D.rep.bytes;
    D.bytes = D.doc_bytes + align_up(((size_t)ndocs + 1) * 4, 256);
    return D;
}

static inline bool docrep_args_valid(int32_t min_len, int32_t mode, int32_t scope, const uint32_t *spans, int64_t capacity, const int64_t *count_out)
{
    return min_len >= 1 && (mode == REP_MODE_ALL || mode == REP_MODE_KEEP_FIRST) && (scope == DOCREP_ANY || scope == DOCREP_OTHER) &&
           capacity >= 0 && count_out && (capacity == 0 || spans);
}

template <int MODE>
static int launch_docrep_mark(int scope, unsigned g, hipStream_t st, const uint32_t *dSA, int64_t n, const uint32_t *lcps, const uint32_t *dsv,
                               const uint32_t *dev, uint32_t k_min, const uint32_t *carry, uint8_t *flag)
{
    if (scope == DOCREP_ANY)
        PROF(KC_REP_LR, n, st, hipLaunchKernelGGL((k_docrep_mark<MODE, DOCREP_ANY>), dim3(g), dim3(REP_THREADS), 0, st, dSA, n, lcps, dsv, dev, k_min, carry, flag));
    else
        PROF(KC_REP_LR, n, st, hipLaunchKernelGGL((k_docrep_mark<MODE, DOCREP_OTHER>), dim3(g), dim3(REP_THREADS), 0, st, dSA, n, lcps, dsv, dev, k_min, carry, flag));
    return SA_AMD_OK;
}

// ix: the resident text, array and collection (device memory on the current device); dWork: docrep_layout(n, ndocs).bytes,
// 256-byte aligned.  The first `capacity` spans to dSpans, the number of all of them to *count_out (host); account: doc_bytes
// (ndocs words) stand in the work block's doc_bytes slab afterwards.  Arguments checked by the caller.  Blocks until done.
static int doc_repeats_device(const sa_amd_index &ix, int32_t min_len, int32_t mode, int32_t scope, uint32_t *dSpans, int64_t capacity,
                              int64_t *count_out, bool account, void *dWork, int64_t work_bytes, hipStream_t st)
{
    const int64_t n = ix.n;
    sa_amd_doc_repeat_stats ds;
    memset(&ds, 0, sizeof(ds));
    ds.docs_touched = account ? 0 : -1;
    g_last_doc_repeat_stats = ds;
    sa_amd_repeat_stats rs;
    memset(&rs, 0, sizeof(rs));
    g_last_repeat_stats = rs;
    sa_amd_lcp_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_lcp_stats = stats;
    const DocRepLayout D = docrep_layout(ix.n, ix.ndocs);
    const LcpLayout &L = D.rep.lcp;
    if (work_bytes < (int64_t)D.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    const Tuning tn = route_tuning();
    const int rb0 = g_readbacks;
    char *base = (char *)dWork;
    uint32_t *dDocBytes = (uint32_t *)(base + D.doc_bytes);
    { const int rcf = lcp_front(ix.text(), ix.sa(), n, dWork, L, st, tn, stats); if (rcf) return rcf; }
    stats.readbacks = g_readbacks - rb0;
    g_last_lcp_stats = stats;
    if (account) HIP_TRY(hipMemsetAsync(dDocBytes, 0, (size_t)ix.ndocs * 4, st));
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        *count_out = 0;
        rs.longest_pos = -1;
        rs.readbacks = ds.readbacks = g_readbacks - rb0;
        g_last_repeat_stats = rs;
        g_last_doc_repeat_stats = ds;
        return SA_AMD_OK;
    }

    uint32_t *err = (uint32_t *)(base + L.ctl);
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl + REP_CTL_OFF);
    unsigned long long *dctl = (unsigned long long *)(base + L.ctl + DOCREP_CTL_OFF);
    const uint32_t *plcp = (const uint32_t *)(base + L.phi);
    uint32_t *alt = (uint32_t *)(base + L.alt);
    const size_t ae = L.alt_elems;
    const int64_t tiles = ceil_div(n, REP_TILE);
    if ((size_t)tiles * (DOCREP_AGG + DOCREP_CARRY + 1) > ae) return SA_AMD_EINTERNAL;      // (10 words per 2048 slots: never)
    uint32_t *lcps = alt, *dsv = alt + ae, *dev = alt + 2 * ae;
    uint32_t *agg = alt + 3 * ae, *carry = agg + (size_t)tiles * DOCREP_AGG, *cnt = carry + (size_t)tiles * DOCREP_CARRY;
    uint32_t *tile_max = (uint32_t *)(base + L.tiles);
    uint8_t *flag = (uint8_t *)(base + D.rep.lr);
    const uint32_t k_min = (uint32_t)min_len, M = ix.ndocs + 1u;
    const unsigned g = (unsigned)tiles;

    // ---- slot pass, spine, mark: the flag bytes ----
    HIP_TRY(hipMemsetAsync(flag, 0, (size_t)n, st));
    {
        // the sampled top level of the offsets, as launch_doc_of cuts it; the workgroups are resident ones that walk over the tiles
        const uint32_t stride = (uint32_t)ceil_div((int64_t)M, DOC_SAMPLES), ns = (uint32_t)ceil_div((int64_t)M, stride);
        int64_t sg = (int64_t)cu_count() * 4;
        if (sg > tiles) sg = tiles;
        PROF(KC_REP_LR, n, st, hipLaunchKernelGGL(k_docrep_slots, dim3((unsigned)sg), dim3(REP_THREADS), 0, st, ix.sa(), n, plcp, ix.doc_off(), M, stride, ns, k_min,
                                                  lcps, dsv, dev, agg, ctl, dctl));
    }
    PROF(KC_REP_LR, tiles, st, hipLaunchKernelGGL(k_docrep_seg_spine, dim3(4), dim3(REP_SPINE_THREADS), 0, st, (const uint32_t *)agg, tiles, carry));
    {
        const int rcm = mode == REP_MODE_ALL ? launch_docrep_mark<REP_MODE_ALL>(scope, g, st, ix.sa(), n, lcps, dsv, dev, k_min, carry, flag)
                                             : launch_docrep_mark<REP_MODE_KEEP_FIRST>(scope, g, st, ix.sa(), n, lcps, dsv, dev, k_min, carry, flag);
        if (rcm) return rcm;
    }

    // ---- spans: the flagged positions reach k bytes, as those of KEEP_FIRST do ----
    { const int rcl = launch_spans<REP_MODE_KEEP_FIRST>(flag, n, k_min, tile_max, cnt, dSpans, capacity, ctl, st); if (rcl) return rcl; }

    // ---- per-document accounting (tile_max: still the exclusive running maximum of the tiles' reach) ----
    if (account) {
        PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL(k_docrep_account, dim3(g), dim3(REP_THREADS), 0, st, (const uint8_t *)flag, n, k_min,
                                                     (const uint32_t *)tile_max, ix.doc_off(), M, dDocBytes));
        int64_t tg = ceil_div((int64_t)ix.ndocs, REP_THREADS);
        if (tg > 4096) tg = 4096;
        PROF(KC_MISC, (int64_t)ix.ndocs, st, hipLaunchKernelGGL(k_docrep_touched, dim3((unsigned)tg), dim3(REP_THREADS), 0, st, (const uint32_t *)dDocBytes,
                                                                (int64_t)ix.ndocs, &dctl[DOCREP_C_TOUCHED]));
    }

    // ---- one read-back: the sort's error word and the counters ----
    uint32_t head[(DOCREP_CTL_OFF + DOCREP_C_WORDS * 8) / 4];
    { const int rcw = read_words(head, err, sizeof(head), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    if (head[0]) return SA_AMD_EINTERNAL;
    unsigned long long cw[REP_C_WORDS + DOCREP_C_WORDS];
    memcpy(cw, (const char *)head + REP_CTL_OFF, sizeof(cw));
    rs.longest = (int64_t)(cw[REP_C_BEST] >> 32);
    rs.longest_pos = rs.longest > 0 ? (int64_t)(uint32_t)~(uint32_t)cw[REP_C_BEST] : -1;
    rs.lcp_sum = (int64_t)cw[REP_C_SUM];
    rs.distinct_substrings = n * (n + 1) / 2 - rs.lcp_sum;
    rs.spans = ds.spans = (int64_t)cw[REP_C_SPANS];
    rs.covered_bytes = ds.covered_bytes = (int64_t)cw[REP_C_COVERED];
    rs.flagged = ds.flagged = (int64_t)cw[REP_C_FLAGGED];
    ds.members = (int64_t)cw[REP_C_WORDS + DOCREP_C_MEMBERS];
    if (account) ds.docs_touched = (int64_t)cw[REP_C_WORDS + DOCREP_C_TOUCHED];
    *count_out = rs.spans;
    rs.readbacks = ds.readbacks = g_readbacks - rb0;
    g_last_repeat_stats = rs;
    g_last_doc_repeat_stats = ds;
    stats.readbacks = rs.readbacks;
    g_last_lcp_stats = stats;
    return SA_AMD_OK;
}

// host pointers; the work block and the spans' slab come from the pool, on the null stream as the index's other routes
static int doc_repeats_index(const sa_amd_index &ix, int32_t min_len, int32_t mode, int32_t scope, uint32_t *spans, int64_t capacity, int64_t *count_out,
                             uint32_t *doc_bytes)
{
    CappedRows rows(capacity, repeat_spans_bound(ix.n, min_len));
    PooledScope sc(ix.device, false);
    const DocRepLayout D = docrep_layout(ix.n, ix.ndocs);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), D.bytes, rows.bytes());
    uint32_t *dOut = (uint32_t *)sc.take(rows.bytes());
    if (sc.rc == SA_AMD_OK)
        sc.rc = doc_repeats_device(ix, min_len, mode, scope, dOut, rows.cap, &rows.count, doc_bytes != nullptr, in.dW, (int64_t)in.wb, sc.st);
    if (doc_bytes) sc.down(doc_bytes, (const char *)in.dW + D.doc_bytes, (size_t)ix.ndocs * 4);
    return rows.finish(sc, spans, dOut, count_out);
}

}  // namespace sa
