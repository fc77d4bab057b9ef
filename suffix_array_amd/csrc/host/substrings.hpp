// host/substrings.hpp -- repeated substrings from a device-resident text and suffix array (kernels/substrings.hpp, DESIGN.md
// section 19): work-block layout, the device entry point's sequence and the host-pointer routes.
//
// Buffers.  The work block is the LCP array's block | LCPV (n + 1 entries) | SKEYS (one 8-byte buffer) | SVALS (two 4-byte buffers).
//   LCP build     the LCP block as host/lcp.hpp uses it; at its end PLCP stands in the Φ buffer and k_lcp_gather writes the LCP
//                 array in slot order to LCPV, which stays to the end.  From here on the Φ buffer and the LCP block's four
//                 n-entry buffers A0 .. A3 are free.
//   stage 1       psl in A0, nsl in A1 (both stay to the end: the gather reads them), the levels of minima in A2.
//   node pass     the tiles' counts in the LCP block's tile words.  Ranked orders: the candidates' keys (8 bytes) in A2 | A3 --
//                 the levels are dead --, their slots in the Φ buffer (stays to the end).
//   select        the digit histograms in the sort's spine slab, which no sort is using yet.
//   cut           the tiles' two counts in the second SVALS buffer; the kept pairs to SKEYS and the first SVALS buffer.
//   sort          SKEYS / first SVALS <-> A2 | A3 (the candidates' keys are dead) / second SVALS (the counts are dead); spine
//                 and granules of the LCP block.
// Read-backs, all through read_words and counted: the LCP build's; one behind the node pass (ORDER_ALL: the last one); ranked:
// one per select pass and one at the end (the sort's error word and the cut's totals).
//
// substrings_run is the sequence, written once for this file's entry points (Docs = SubNoDocs: the kernels' DF = false, the
// arithmetic of section 19) and for host/doc_substrings.hpp, whose Docs adds the document table between stage 1 and the node pass.
#pragma once
#include "lcp.hpp"
#include "lz.hpp"
#include "../kernels/substrings.hpp"

namespace sa {

static thread_local sa_amd_substr_stats g_last_substr_stats;

constexpr int SUB_CTL_OFF = LZ_CTL_OFF;     // byte offset of the control words in the LCP control slab: stage 1 counts into the first three
static_assert(LCP_CTL_OFF + LCP_C_WORDS * 8 <= SUB_CTL_OFF && SUB_CTL_OFF + SUB_C_WORDS * 8 <= 256, "control slab");
static_assert(REP_TILE == LCP_TILE, "the tiles' counts of the node pass live in the LCP block's tile words");
static_assert(SUB_ORDER_ALL == SA_AMD_SUBSTR_ALL && SUB_ORDER_COUNT == SA_AMD_SUBSTR_BY_COUNT && SUB_ORDER_LENGTH == SA_AMD_SUBSTR_BY_LENGTH &&
              SUB_ORDER_COVER == SA_AMD_SUBSTR_BY_COVER, "the kernels take the ABI's order");
constexpr int SUB_SELECT_MAX = 8;           // 8-bit digits of a 64-bit key
static_assert((size_t)SUB_SELECT_MAX * 256 * 4 <= SortScratch::SPINE_BYTES, "the select's histograms live in the spine slab");

struct SubLayout { LcpLayout lcp; size_t lcpv, skeys, svals, bytes; };
static SubLayout sub_layout(int32_t n)
{
    SubLayout S;
    S.lcp = lcp_layout(n);
    const size_t ae = S.lcp.alt_elems;
    S.lcpv = S.lcp.bytes;
    S.skeys = S.lcpv + align_up(ae * 4, 256);
    S.svals = S.skeys + align_up(ae * 8, 256);
    S.bytes = S.svals + align_up(2 * ae * 4, 256);
    return S;
}

static inline int64_t substrings_bound(int64_t n) { return n > 1 ? n - 1 : 0; }

// what needs no device: the query's ranges and the output arguments
static bool sub_args_ok(const sa_amd_substr_query *q, const uint32_t *rows, int64_t capacity, const int64_t *total)
{
    if (!q || !total || capacity < 0 || (capacity > 0 && !rows)) return false;
    if (q->min_len < 1 || q->max_len < 0 || (q->max_len != 0 && q->max_len < q->min_len) || q->min_count < 2) return false;
    if (q->order < SA_AMD_SUBSTR_ALL || q->order > SA_AMD_SUBSTR_BY_COVER) return false;
    return q->order == SA_AMD_SUBSTR_ALL || q->k >= 1;
}

// rows the caller's buffers and the query can take: no more than exist, whatever the capacity
static int64_t sub_row_cap(int64_t n, const sa_amd_substr_query &q, int64_t capacity)
{
    int64_t cap = substrings_bound(n);
    if (q.order != SA_AMD_SUBSTR_ALL && q.k < cap) cap = q.k;
    return capacity < cap ? capacity : cap;
}

// the Docs of a run without documents: no table, DF = false in the kernels
struct SubNoDocs {
    static constexpr bool on = false;
    int table(const uint32_t *, int64_t, const LzLevels &, char *, hipStream_t) { return SA_AMD_OK; }
    SubDf df() const { return SubDf{ nullptr, 0u, nullptr, nullptr }; }
    void counters(const uint32_t *) {}
};

// dT, dSA (n + 1 entries, SA[0] = n): device memory on the current device; dWork: the block of layout S (checked by the caller,
// as is the query Q), 256-byte aligned.  The first `capacity` rows of the query to dRows (4 words a row) and dPos (may be null),
// the number of all of them to *total_out (host); the counters to ss, which the caller has cleared.  docs: see SubNoDocs; its
// table is built while the levels of minima stand in A2, its counters are read from the node pass's read-back.  Blocks until done.
template <class Docs>
static int substrings_run(const uint8_t *dT, const uint32_t *dSA, int32_t n32, const sa_amd_substr_query &Q, uint32_t *dRows, uint32_t *dPos,
                          int64_t capacity, int64_t *total_out, void *dWork, const SubLayout &S, hipStream_t st, sa_amd_substr_stats &ss, Docs &docs)
{
    const int64_t n = n32;
    sa_amd_lcp_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_lcp_stats = stats;
    const LcpLayout &L = S.lcp;
    const bool ranked = Q.order != SA_AMD_SUBSTR_ALL;
    const Tuning tn = route_tuning();
    const int rb0 = g_readbacks;

    // ---- the LCP array, in slot order, into the block ----
    { const int rcf = lcp_front(dT, dSA, n, dWork, L, st, tn, stats); if (rcf) return rcf; }
    stats.readbacks = g_readbacks - rb0;
    g_last_lcp_stats = stats;
    if (n == 0) {
        *total_out = 0;
        ss.readbacks = g_readbacks - rb0;
        return SA_AMD_OK;
    }
    char *base = (char *)dWork;
    uint32_t *err = (uint32_t *)(base + L.ctl);
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl + SUB_CTL_OFF);
    uint32_t *phi = (uint32_t *)(base + L.phi);
    uint32_t *alt = (uint32_t *)(base + L.alt);
    const size_t ae = L.alt_elems;
    uint32_t *lcpv = (uint32_t *)(base + S.lcpv);
    const int64_t N1 = n + 1;
    {
        int64_t gb = ceil_div(N1, 256 * 4);
        if (gb > 65536) gb = 65536;
        PROF(KC_LCP_GATHER, N1, st, hipLaunchKernelGGL(k_lcp_gather, dim3((unsigned)gb), dim3(256), 0, st, dSA, n, (const uint32_t *)phi, lcpv));
    }

    // ---- stage 1 over LCP[0 .. n]: the nearest "<=" on the left, the nearest "<" on the right ----
    uint32_t *psl = alt, *nsl = alt + ae;
    { const int rcn = lz_nsv<true>(lcpv, N1, psl, nsl, alt + 2 * ae, nullptr, nullptr, ctl, st); if (rcn) return rcn; }
    { const int rcd = docs.table(lcpv, N1, lz_levels(N1, alt + 2 * ae), base, st); if (rcd) return rcd; }

    // ---- node pass: counts per tile, their running sum, rows (ORDER_ALL) or candidates (ranked) in slot order ----
    SubQuery q;
    q.min_len = (uint32_t)Q.min_len; q.max_len = (uint32_t)Q.max_len; q.min_count = (uint32_t)Q.min_count; q.order = Q.order;
    uint32_t *cnt = (uint32_t *)(base + L.tiles);
    unsigned long long *ckeys = (unsigned long long *)(alt + 2 * ae);
    uint32_t *cslots = phi;
    const int64_t tiles = ceil_div(N1, REP_TILE);
    PROF(KC_REP_SPANS, N1, st, hipLaunchKernelGGL((k_sub_nodes<0, Docs::on>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, (const uint32_t *)lcpv,
                                                  (const uint32_t *)psl, (const uint32_t *)nsl, dSA, n, q, cnt, dRows, dPos, capacity, ckeys, cslots, ctl,
                                                  docs.df()));
    PROF(KC_REP_SPANS, tiles, st, hipLaunchKernelGGL(k_rep_sum_spine, dim3(1), dim3(REP_SPINE_THREADS), 0, st, cnt, tiles, &ctl[SUB_C_TOTAL]));
    PROF(KC_REP_SPANS, N1, st, hipLaunchKernelGGL((k_sub_nodes<1, Docs::on>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, (const uint32_t *)lcpv,
                                                  (const uint32_t *)psl, (const uint32_t *)nsl, dSA, n, q, cnt, dRows, dPos, capacity, ckeys, cslots, ctl,
                                                  docs.df()));
    uint32_t head[256 / 4];
    { const int rcw = read_words(head, err, sizeof(head), st); if (rcw) return rcw; }
    unsigned long long cw[SUB_C_WORDS];
    memcpy(cw, (const char *)head + SUB_CTL_OFF, sizeof(cw));
    ss.unresolved = (int64_t)cw[LZ_C_UNRES];
    ss.far_steps = (int64_t)cw[LZ_C_HSTEPS];
    ss.far_max = (int64_t)cw[LZ_C_HMAX];
    ss.nodes = (int64_t)cw[SUB_C_NODES];
    ss.selected = (int64_t)cw[SUB_C_SELECTED];
    ss.distinct_all = (int64_t)cw[SUB_C_DALL];
    ss.distinct_selected = (int64_t)cw[SUB_C_DSEL];
    docs.counters(head);
    if ((int64_t)cw[SUB_C_TOTAL] != ss.selected || ss.selected > substrings_bound(n)) return SA_AMD_EINTERNAL;
    const int64_t m = ss.selected;
    const int64_t kept = ranked ? (Q.k < m ? Q.k : m) : m;

    if (ranked && kept > 0) {
        // ---- radix select: the cut key, digit by digit from the highest one the largest key has ----
        const unsigned long long maxkey = cw[SUB_C_MAXKEY];
        const int width = bit_length((uint64_t)maxkey);
        unsigned long long above = 0, at_cut = 0;           // (k >= selected: everything is above the cut)
        int64_t need = 0;
        if (Q.k < m) {
            uint32_t *hist = (uint32_t *)(base + L.spine);
            HIP_TRY(hipMemsetAsync(hist, 0, (size_t)SUB_SELECT_MAX * 256 * 4, st));
            int64_t hb = ceil_div(m, (int64_t)SUB_HIST_THREADS * 8);
            if (hb > 4096) hb = 4096;
            unsigned long long prefix = 0;
            need = Q.k;
            int shift = 8 * ((width - 1) / 8);
            for (;; shift -= 8) {
                if (ss.select_passes >= SUB_SELECT_MAX) return SA_AMD_EINTERNAL;
                uint32_t *h = hist + (size_t)ss.select_passes * 256;
                PROF(KC_REP_SPANS, m, st, hipLaunchKernelGGL(k_sub_hist, dim3((unsigned)hb), dim3(SUB_HIST_THREADS), 0, st,
                                                             (const unsigned long long *)ckeys, m, shift + 8, prefix, shift, h));
                uint32_t hh[256];
                { const int rcw = read_words(hh, h, sizeof(hh), st); if (rcw) return rcw; }
                ++ss.select_passes;
                int d = 255;
                int64_t over = 0;
                while (d > 0 && over + (int64_t)hh[d] < need) { over += hh[d]; --d; }
                if (over + (int64_t)hh[d] < need) return SA_AMD_EINTERNAL;       // (fewer candidates under the prefix than the pass before counted)
                need -= over;
                prefix = (prefix << 8) | (unsigned long long)d;
                if ((int64_t)hh[d] == need || shift == 0) break;                 // the whole bin is kept, or the key is complete
            }
            at_cut = prefix << shift;
            above = (prefix + 1) << shift;                  // (keys are below 2^62: no wrap)
        }

        // ---- the kept candidates in slot order, as (~key, candidate index); the sort; the rows ----
        unsigned long long *skeys = (unsigned long long *)(base + S.skeys);
        uint32_t *svals = (uint32_t *)(base + S.svals), *svals2 = svals + ae;
        const int64_t ctiles = ceil_div(m, REP_TILE);
        uint32_t *cnt_a = svals2, *cnt_e = svals2 + ctiles;
        PROF(KC_REP_SPANS, m, st, hipLaunchKernelGGL((k_sub_cut<0>), dim3((unsigned)ctiles), dim3(REP_THREADS), 0, st, (const unsigned long long *)ckeys, m,
                                                     above, at_cut, need, cnt_a, cnt_e, skeys, svals));
        PROF(KC_REP_SPANS, ctiles, st, hipLaunchKernelGGL(k_rep_sum_spine, dim3(1), dim3(REP_SPINE_THREADS), 0, st, cnt_a, ctiles, &ctl[SUB_C_ABOVE]));
        PROF(KC_REP_SPANS, ctiles, st, hipLaunchKernelGGL(k_rep_sum_spine, dim3(1), dim3(REP_SPINE_THREADS), 0, st, cnt_e, ctiles, &ctl[SUB_C_ATCUT]));
        PROF(KC_REP_SPANS, m, st, hipLaunchKernelGGL((k_sub_cut<1>), dim3((unsigned)ctiles), dim3(REP_THREADS), 0, st, (const unsigned long long *)ckeys, m,
                                                     above, at_cut, need, cnt_a, cnt_e, skeys, svals));
        const SortScratch sc = SortScratch::make(base + L.spine, base + L.status, err);
        SortJob<uint64_t> job{ (uint64_t *)skeys, svals, (uint64_t *)ckeys, svals2, kept, 0, width };
        SortResult<uint64_t> res;
        { const int rcs = sort_pairs(job, sc, st, tn, &res); if (rcs) return rcs; }
        ss.sorted = kept;
        const int64_t wr = kept < capacity ? kept : capacity;
        if (wr > 0)
            PROF(KC_REP_SPANS, wr, st, hipLaunchKernelGGL((k_sub_gather<Docs::on>), dim3((unsigned)ceil_div(wr, SUB_HIST_THREADS)), dim3(SUB_HIST_THREADS), 0, st,
                                                          (const uint32_t *)res.vals, wr, m, (const uint32_t *)cslots, (const uint32_t *)lcpv,
                                                          (const uint32_t *)psl, (const uint32_t *)nsl, dSA, n, dRows, dPos, docs.df()));
        { const int rcw = read_words(head, err, sizeof(head), st); if (rcw) return rcw; }
        memcpy(cw, (const char *)head + SUB_CTL_OFF, sizeof(cw));
        if (head[0]) return SA_AMD_EINTERNAL;               // a look-back of the sort gave up (never seen; never a silently wrong order)
        const int64_t at = (int64_t)cw[SUB_C_ATCUT];
        if ((int64_t)cw[SUB_C_ABOVE] + (at < need ? at : need) != kept) return SA_AMD_EINTERNAL;
    }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    *total_out = kept;
    ss.readbacks = g_readbacks - rb0;
    return SA_AMD_OK;
}

// dWork: sub_layout(n).bytes, 256-byte aligned; the rest as substrings_run.  The calling thread's statistics are this call's,
// all zero when it fails.
static int substrings_device(const uint8_t *dT, const uint32_t *dSA, int32_t n32, const sa_amd_substr_query *query, uint32_t *dRows, uint32_t *dPos,
                             int64_t capacity, int64_t *total_out, void *dWork, int64_t work_bytes, hipStream_t st)
{
    sa_amd_substr_stats ss;
    memset(&ss, 0, sizeof(ss));
    g_last_substr_stats = ss;
    sa_amd_lcp_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_lcp_stats = stats;
    const SubLayout S = sub_layout(n32);
    if (work_bytes < (int64_t)S.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    if (!sub_args_ok(query, dRows, capacity, total_out)) return SA_AMD_EINVAL;
    SubNoDocs none;
    const int rc = substrings_run(dT, dSA, n32, *query, dRows, dPos, capacity, total_out, dWork, S, st, ss, none);
    if (rc == SA_AMD_OK) g_last_substr_stats = ss;
    return rc;
}

// Over a resident text and array, the outputs in two slabs of the scope's block: the first min(capacity, total) rows and their
// pos come back.  The convention is CappedRows' (scope.hpp) -- slabs for min(capacity, bound) rows, min(count, cap) rows down,
// *total written only behind a successful wait --, written out here because CappedRows is one slab of 8-byte rows and this
// route has 16-byte rows and a parallel 4-byte array that may be absent.  in.dW: the scope's first slab, at least sub_layout(n).bytes.
static size_t sub_rows_bytes(int64_t cap) { return (size_t)cap * 16 + 16; }
static size_t sub_pos_bytes(int64_t cap) { return (size_t)cap * 4 + 16; }
static int substrings_resident(PooledScope &sc, const Inputs &in, int32_t n, const sa_amd_substr_query *q, uint32_t *rows, uint32_t *pos, int64_t cap,
                               int64_t *total)
{
    uint32_t *dRows = (uint32_t *)sc.take(sub_rows_bytes(cap)), *dPos = (uint32_t *)sc.take(sub_pos_bytes(cap));
    int64_t count = 0;
    if (sc.rc == SA_AMD_OK)
        sc.rc = substrings_device(in.dT, in.dSA, n, q, dRows, pos ? dPos : nullptr, cap, &count, in.dW, (int64_t)in.wb, sc.st);
    const int64_t wr = count < cap ? count : cap;
    if (wr > 0) sc.down(rows, dRows, (size_t)wr * 16);
    if (wr > 0 && pos) sc.down(pos, dPos, (size_t)wr * 4);
    if (sc.finish() == SA_AMD_OK) *total = count;
    return sc.rc;
}

// host buffers: the text goes up; the array is built on the device and stays there (SA == nullptr) or the caller's goes up
static int substrings_host(const uint8_t *T, int32_t n, const uint32_t *SA, const sa_amd_substr_query *q, uint32_t *rows, uint32_t *pos, int64_t capacity,
                           int64_t *total)
{
    if (n < 0 || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (!sub_args_ok(q, rows, capacity, total)) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    const int64_t cap = sub_row_cap(n, *q, capacity);
    PooledScope sc(pick_device(), true);
    const Inputs in = upload_inputs(sc, T, n, SA, sub_layout(n).bytes, align_up(sub_rows_bytes(cap), 256) + align_up(sub_pos_bytes(cap), 256));
    return substrings_resident(sc, in, n, q, rows, pos, cap, total);
}

// the index's resident text and array: only the work block and the outputs come from the pool; on the null stream
static int32_t substrings_index(const sa_amd_index &ix, const sa_amd_substr_query *q, uint32_t *rows, uint32_t *pos, int64_t capacity, int64_t *total)
{
    if (!sub_args_ok(q, rows, capacity, total)) return SA_AMD_EINVAL;
    const int64_t cap = sub_row_cap(ix.n, *q, capacity);
    PooledScope sc(ix.device, false);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), sub_layout(ix.n).bytes, align_up(sub_rows_bytes(cap), 256) + sub_pos_bytes(cap));
    return substrings_resident(sc, in, ix.n, q, rows, pos, cap, total);
}

}  // namespace sa
