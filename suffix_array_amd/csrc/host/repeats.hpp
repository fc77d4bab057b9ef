// host/repeats.hpp -- longest-repeat array and duplicate spans from a device-resident text and suffix array
// (kernels/repeats.hpp): work-block layout, the device entry points' sequence and the host-pointer routes.
#pragma once
#include "lcp.hpp"
#include "../kernels/repeats.hpp"

namespace sa {

static_assert(REP_THREADS == LCP_THREADS, "the span kernels use lcp_block_add");
static_assert(REP_TILE == LCP_TILE, "the tile maxima of the reach live in the LCP block's tile words");

static thread_local sa_amd_repeat_stats g_last_repeat_stats;

constexpr int REP_CTL_OFF = 128;           // byte offset of the REP_C_* words in the LCP control slab (behind the LCP_C_* words)
static_assert(LCP_CTL_OFF + LCP_C_WORDS * 8 <= REP_CTL_OFF && REP_CTL_OFF + REP_C_WORDS * 8 <= 256, "control slab");

// layout of the work block: the LCP array's block | one n-entry buffer (LR in mode ALL, the flag bytes in mode KEEP_FIRST).
// After the front end the LCP block's four n-entry buffers are free: the binned scatter's pairs (LR), then the LCP values in
// slot order, the tiles' words of the segmented minimum and the span counts per tile.
struct RepLayout { LcpLayout lcp; size_t lr, bytes; };
static RepLayout rep_layout(int32_t n)
{
    RepLayout R;
    R.lcp = lcp_layout(n);
    R.lr = R.lcp.bytes;
    R.bytes = R.lr + align_up(((size_t)n + 1) * 4, 256);
    return R;
}

static inline int64_t repeat_spans_bound(int64_t n, int64_t min_len) { return (n + 1) / (min_len + 1); }

// The span passes over src (LR in mode ALL, the flag bytes in mode KEEP_FIRST): tile maxima of the reach, their running
// maximum, the starts per tile, their running sum (the total to ctl[REP_C_SPANS]) and the ordered compaction.
template <int MODE>
static int launch_spans(const void *src, int64_t n, uint32_t k_min, uint32_t *tile_max, uint32_t *cnt, uint32_t *dSpans, int64_t capacity,
                        unsigned long long *ctl, hipStream_t st)
{
    const int64_t tiles = ceil_div(n, REP_TILE);
    const unsigned g = (unsigned)tiles;
    PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL((k_rep_reach_max<MODE>), dim3(g), dim3(REP_THREADS), 0, st, src, n, k_min, tile_max));
    PROF(KC_REP_SPANS, tiles, st, hipLaunchKernelGGL(k_lcp_scan_spine, dim3(1), dim3(LCP_SPINE_THREADS), 0, st, tile_max, tiles));
    PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL((k_rep_spans<MODE, 0>), dim3(g), dim3(REP_THREADS), 0, st, src, n, k_min,
                                                 (const uint32_t *)tile_max, cnt, dSpans, capacity, ctl));
    PROF(KC_REP_SPANS, tiles, st, hipLaunchKernelGGL(k_rep_sum_spine, dim3(1), dim3(REP_SPINE_THREADS), 0, st, cnt, tiles, &ctl[REP_C_SPANS]));
    PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL((k_rep_spans<MODE, 1>), dim3(g), dim3(REP_THREADS), 0, st, src, n, k_min,
                                                 (const uint32_t *)tile_max, cnt, dSpans, capacity, ctl));
    return SA_AMD_OK;
}

// dT, dSA (n + 1 entries, SA[0] = n): device memory on the current device; dWork: rep_layout(n).bytes, 256-byte aligned.
// !spans: the longest-repeat array (n entries) to dLR and nothing else.  spans: those of (min_len, mode), the first `capacity` of
// them to dSpans, the number of all of them to *count_out (host).  Blocks until done.
static int repeats_device(const uint8_t *dT, const uint32_t *dSA, int32_t n32, bool spans, uint32_t *dLR, int32_t min_len, int32_t mode,
                          uint32_t *dSpans, int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes, hipStream_t st)
{
    const int64_t n = n32;
    sa_amd_repeat_stats rs;
    memset(&rs, 0, sizeof(rs));
    g_last_repeat_stats = rs;
    sa_amd_lcp_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_lcp_stats = stats;
    const RepLayout R = rep_layout(n32);
    const LcpLayout &L = R.lcp;
    if (work_bytes < (int64_t)R.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    if (spans && (min_len < 1 || (mode != REP_MODE_ALL && mode != REP_MODE_KEEP_FIRST) || capacity < 0 || !count_out)) return SA_AMD_EINVAL;
    const Tuning tn = route_tuning();
    const int rb0 = g_readbacks;
    { const int rcf = lcp_front(dT, dSA, n, dWork, L, st, tn, stats); if (rcf) return rcf; }
    stats.readbacks = g_readbacks - rb0;
    g_last_lcp_stats = stats;
    if (n == 0) {
        if (spans) *count_out = 0;
        rs.longest_pos = -1;
        rs.readbacks = g_readbacks - rb0;
        g_last_repeat_stats = rs;
        return SA_AMD_OK;
    }

    char *base = (char *)dWork;
    uint32_t *err = (uint32_t *)(base + L.ctl);
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl + REP_CTL_OFF);
    const uint32_t *plcp = (const uint32_t *)(base + L.phi);
    uint32_t *alt = (uint32_t *)(base + L.alt);
    const size_t ae = L.alt_elems;
    uint32_t *lrbuf = (uint32_t *)(base + R.lr);
    const int64_t tiles = ceil_div(n, REP_TILE);
    const uint32_t k_min = spans ? (uint32_t)min_len : 1u;
    const bool keep_first = spans && mode == REP_MODE_KEEP_FIRST;

    // ---- slot pass: LR (or, KEEP_FIRST, the LCP values in slot order), the sum, the maximum and where it is first attained ----
    if (keep_first) {
        uint32_t *lcps = alt, *agg = alt + ae, *carry = alt + 2 * ae;
        uint8_t *flag = (uint8_t *)lrbuf;
        HIP_TRY(hipMemsetAsync(flag, 0, (size_t)n, st));
        PROF(KC_REP_LR, n, st, hipLaunchKernelGGL((k_rep_slots<REP_OUT_SLOTS>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, dSA, n, plcp,
                                                  lcps, (uint32_t *)nullptr, k_min, agg, ctl));
        PROF(KC_REP_LR, tiles, st, hipLaunchKernelGGL(k_rep_seg_spine, dim3(2), dim3(REP_SPINE_THREADS), 0, st, (const uint32_t *)agg, tiles, carry));
        PROF(KC_REP_LR, n, st, hipLaunchKernelGGL(k_rep_mark, dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, dSA, n, (const uint32_t *)lcps,
                                                  k_min, (const uint32_t *)carry, flag));
    } else {
        uint32_t *dst = spans ? lrbuf : dLR;
        if (binned(n, n, tn)) {
            // the random 4-byte stores of LR go through the binned scatter, as those of Φ do: the pass writes the pairs in slot order
            const SortScratch ss = SortScratch::make(base + L.spine, base + L.status, err);
            PROF(KC_REP_LR, n, st, hipLaunchKernelGGL((k_rep_slots<REP_OUT_PAIRS>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, dSA, n, plcp,
                                                      alt, alt + ae, k_min, (uint32_t *)nullptr, ctl));
            sa_amd_stats local;
            memset(&local, 0, sizeof(local));
            const int rcs = scatter_binned(ss, dst, alt, alt + ae, alt + 2 * ae, alt + 3 * ae, n, n, st, &local, tn);
            if (rcs) return rcs;
        } else {
            PROF(KC_REP_LR, n, st, hipLaunchKernelGGL((k_rep_slots<REP_OUT_PLAIN>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, dSA, n, plcp,
                                                      dst, (uint32_t *)nullptr, k_min, (uint32_t *)nullptr, ctl));
        }
    }

    // ---- spans: running maximum of the reach, starts per tile, ordered compaction ----
    if (spans) {
        uint32_t *tile_max = (uint32_t *)(base + L.tiles), *cnt = alt + 3 * ae;
        const int rcl = keep_first ? launch_spans<REP_MODE_KEEP_FIRST>(lrbuf, n, k_min, tile_max, cnt, dSpans, capacity, ctl, st)
                                   : launch_spans<REP_MODE_ALL>(lrbuf, n, k_min, tile_max, cnt, dSpans, capacity, ctl, st);
        if (rcl) return rcl;
    }

    // ---- one read-back: the sort's error word and the counters ----
    uint32_t head[(REP_CTL_OFF + REP_C_WORDS * 8) / 4];
    { const int rcw = read_words(head, err, sizeof(head), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    if (head[0]) return SA_AMD_EINTERNAL;           // a look-back of the binned scatter's sort gave up (never seen; never a silent wrong LR)
    unsigned long long cw[REP_C_WORDS];
    memcpy(cw, (const char *)head + REP_CTL_OFF, sizeof(cw));
    rs.longest = (int64_t)(cw[REP_C_BEST] >> 32);
    rs.longest_pos = rs.longest > 0 ? (int64_t)(uint32_t)~(uint32_t)cw[REP_C_BEST] : -1;
    rs.lcp_sum = (int64_t)cw[REP_C_SUM];
    rs.distinct_substrings = n * (n + 1) / 2 - rs.lcp_sum;
    if (spans) {
        rs.spans = (int64_t)cw[REP_C_SPANS];
        rs.covered_bytes = (int64_t)cw[REP_C_COVERED];
        rs.flagged = (int64_t)cw[REP_C_FLAGGED];
        *count_out = rs.spans;
    }
    rs.readbacks = g_readbacks - rb0;
    g_last_repeat_stats = rs;
    stats.readbacks = rs.readbacks;
    g_last_lcp_stats = stats;
    return SA_AMD_OK;
}

// Either form over a resident text and array, the output in a slab of the scope's block: LR (4 n bytes) or the first rows.cap
// spans come back.  in.dW: the scope's first slab, at least rep_layout(n).bytes.
static int repeats_resident(PooledScope &sc, const Inputs &in, int32_t n, bool spans, uint32_t *LR, int32_t min_len, int32_t mode, uint32_t *out_spans,
                            CappedRows &rows, int64_t *count_out)
{
    uint32_t *dOut = (uint32_t *)sc.take(spans ? rows.bytes() : ((size_t)n + 1) * 4);
    if (sc.rc == SA_AMD_OK)
        sc.rc = repeats_device(in.dT, in.dSA, n, spans, dOut, min_len, mode, dOut, rows.cap, &rows.count, in.dW, (int64_t)in.wb, sc.st);
    if (spans) return rows.finish(sc, out_spans, dOut, count_out);
    if (n > 0) sc.down(LR, dOut, (size_t)n * 4);
    return sc.finish();
}

// host buffers: the text goes up; the array is built on the device and stays there (SA == nullptr) or the caller's goes up
static int repeats_host(const uint8_t *T, int32_t n, const uint32_t *SA, bool spans, uint32_t *LR, int32_t min_len, int32_t mode, uint32_t *out_spans,
                        int64_t capacity, int64_t *count_out)
{
    if (n < 0 || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (spans && (min_len < 1 || (mode != REP_MODE_ALL && mode != REP_MODE_KEEP_FIRST) || capacity < 0 || !count_out ||
                  (capacity > 0 && !out_spans))) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    CappedRows rows;
    if (spans) rows = CappedRows(capacity, repeat_spans_bound(n, min_len));
    PooledScope sc(pick_device(), true);
    const Inputs in = upload_inputs(sc, T, n, SA, rep_layout(n).bytes, align_up(spans ? rows.bytes() : ((size_t)n + 1) * 4, 256));
    return repeats_resident(sc, in, n, spans, LR, min_len, mode, out_spans, rows, count_out);
}

// the index's resident text and array: only the work block and the output come from the pool; on the null stream
static int32_t repeats_index(const sa_amd_index &ix, bool spans, uint32_t *LR, int32_t min_len, int32_t mode, uint32_t *out_spans, int64_t capacity,
                             int64_t *count_out)
{
    if (spans ? (min_len < 1 || (mode != SA_AMD_REPEATS_ALL && mode != SA_AMD_REPEATS_KEEP_FIRST) || capacity < 0 || !count_out ||
                 (capacity > 0 && !out_spans))
              : (ix.n > 0 && !LR)) return SA_AMD_EINVAL;
    CappedRows rows;
    if (spans) rows = CappedRows(capacity, repeat_spans_bound(ix.n, min_len));
    PooledScope sc(ix.device, false);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), rep_layout(ix.n).bytes, spans ? rows.bytes() : ((size_t)ix.n + 1) * 4);
    return repeats_resident(sc, in, ix.n, spans, LR, min_len, mode, out_spans, rows, count_out);
}

}  // namespace sa
