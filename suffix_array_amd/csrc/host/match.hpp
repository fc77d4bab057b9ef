// host/match.hpp -- matching statistics and shared spans of a query against a device-resident index (kernels/match.hpp,
// DESIGN.md section 15): work-block layout, the two passes and the span passes, the host-pointer routes.
#pragma once
#include "repeats.hpp"
#include "esa.hpp"
#include "index.hpp"
#include "../kernels/match.hpp"

namespace sa {

static thread_local sa_amd_match_stats g_last_match_stats;
static thread_local int32_t g_match_cap = -1;          // sa_amd_match_set_group_cap of the calling thread (-1: MATCH_CAP_DEFAULT)
static thread_local int32_t g_match_lanes = 8;         // sa_amd_match_set_group_lanes of the calling thread: 4, 8 or 16

// layout of the work block: control words | the long list (m entries) | the flag bytes (m) | the span passes' words per tile
struct MatchLayout { size_t ctl, list, flag, tile_max, cnt, bytes; };
static MatchLayout match_layout(int32_t m)
{
    MatchLayout L;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = align_up(off + b, 256); return o; };
    const size_t tiles = (size_t)ceil_div((int64_t)m, REP_TILE) + 1;
    L.ctl = take(256);
    L.list = take(((size_t)m + 1) * 4);
    L.flag = take((size_t)m + 16);
    L.tile_max = take(tiles * 4);
    L.cnt = take(tiles * 4);
    L.bytes = off;
    return L;
}
static_assert((MATCH_C_WORDS + REP_C_WORDS) * 8 <= 256, "control slab");

template <int G>
static void launch_match_tile(const sa_amd_index &ix, const uint8_t *dQ, int64_t m, int64_t C, int ge, uint32_t *dML, uint32_t *dPOS, uint8_t *flag,
                              uint32_t *list, unsigned long long *ctl, hipStream_t st)
{
    const unsigned g = (unsigned)ceil_div(m, MATCH_TILE);
    hipLaunchKernelGGL((k_match_tile<G>), dim3(g), dim3(MATCH_THREADS), (size_t)match_stage_words(ge) * 4, st, ix.text(), ix.sa(), (int64_t)ix.n, ix.bkt(),
                       dQ, m, C, ge, dML, dPOS, flag, list, ctl);
}

// dQ: m bytes on the index's device (any byte address); dWork: match_layout(m).bytes, 256-byte aligned.  !spans: ML and POS
// (either may be nullptr) for cap C.  spans: those of min_len = C, the first `capacity` of them to dSpans, the number of all of
// them to *count_out (host).  Blocks until done.
static int match_device(const sa_amd_index &ix, const uint8_t *dQ, int32_t m32, int32_t C32, bool spans, uint32_t *dML, uint32_t *dPOS,
                        uint32_t *dSpans, int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes, hipStream_t st)
{
    const int64_t m = m32, C = C32;
    const MatchLayout L = match_layout(m32);
    if (m32 < 0 || C32 < 1 || (m > 0 && !dQ)) return SA_AMD_EINVAL;
    if (!dWork || work_bytes < (int64_t)L.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    if (spans && (capacity < 0 || !count_out || (capacity > 0 && !dSpans))) return SA_AMD_EINVAL;
    sa_amd_match_stats ms;
    memset(&ms, 0, sizeof(ms));
    const int cap = g_match_cap < 0 ? MATCH_CAP_DEFAULT : g_match_cap;
    const int G = g_match_lanes;
    ms.positions = m;
    ms.longest_pos = -1;
    ms.route_long = ix.pair() ? 1 : 0;
    ms.group_cap = cap < MATCH_STAGE_MAX ? cap : MATCH_STAGE_MAX;
    ms.group_lanes = G >= 16 ? 16 : (G >= 8 ? 8 : 4);
    ms.tile = MATCH_TILE;
    g_last_match_stats = ms;
    if (m == 0) {
        if (spans) *count_out = 0;
        return SA_AMD_OK;
    }
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const int rb0 = g_readbacks;
    char *base = (char *)dWork;
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl), *rctl = ctl + MATCH_C_WORDS;
    uint32_t *list = (uint32_t *)(base + L.list);
    uint8_t *flag = spans ? (uint8_t *)(base + L.flag) : nullptr;
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));

    // ---- pass 1: the group path ----
    g_prof.begin(KC_MISC, m, st);
    if (ms.group_lanes == 4) launch_match_tile<4>(ix, dQ, m, C, ms.group_cap, dML, dPOS, flag, list, ctl, st);
    else if (ms.group_lanes == 8) launch_match_tile<8>(ix, dQ, m, C, ms.group_cap, dML, dPOS, flag, list, ctl, st);
    else launch_match_tile<16>(ix, dQ, m, C, ms.group_cap, dML, dPOS, flag, list, ctl, st);
    g_prof.end(st);
    LAUNCH_CHECK(st);
    unsigned long long cw[MATCH_C_WORDS + REP_C_WORDS];
    { const int rcw = read_words(cw, ctl, sizeof(cw), st); if (rcw) return rcw; }
    const int64_t longs = (int64_t)(uint32_t)cw[MATCH_C_LONG];
    if (longs > m) return SA_AMD_EINTERNAL;

    // ---- pass 2: one wave per listed position ----
    if (longs > 0) {
        const unsigned g = (unsigned)ceil_div(longs * WAVE, MATCH_THREADS);
        if (ix.pair())
            PROF(KC_MISC, longs, st, hipLaunchKernelGGL((k_match_long<true>), dim3(g), dim3(MATCH_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n, ix.pair(),
                                                        esa_log_p(ix.n), dQ, m, C, (const uint32_t *)list, longs, dML, dPOS, flag, ctl));
        else
            PROF(KC_MISC, longs, st, hipLaunchKernelGGL((k_match_long<false>), dim3(g), dim3(MATCH_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                        (const uint64_t *)nullptr, 0, dQ, m, C, (const uint32_t *)list, longs, dML, dPOS, flag, ctl));
    }

    // ---- spans: the flags are the later copies of the repeat finder's mode KEEP_FIRST (reach = j + C) ----
    if (spans) {
        const int rcl = launch_spans<REP_MODE_KEEP_FIRST>(flag, m, (uint32_t)C32, (uint32_t *)(base + L.tile_max), (uint32_t *)(base + L.cnt), dSpans,
                                                          capacity, rctl, st);
        if (rcl) return rcl;
    }
    if (longs > 0 || spans) { const int rcw = read_words(cw, ctl, sizeof(cw), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    ms.long_positions = longs;
    ms.compared_bytes = (int64_t)cw[MATCH_C_BYTES];
    ms.steps = (int64_t)cw[MATCH_C_STEPS];
    ms.matched = (int64_t)cw[MATCH_C_MATCHED];
    ms.ml_sum = (int64_t)cw[MATCH_C_SUM];
    ms.longest = (int64_t)(cw[MATCH_C_BEST] >> 32);
    ms.longest_pos = ms.longest > 0 ? (int64_t)(uint32_t)~(uint32_t)cw[MATCH_C_BEST] : -1;
    if (spans) {
        ms.spans = (int64_t)cw[MATCH_C_WORDS + REP_C_SPANS];
        ms.covered_bytes = (int64_t)cw[MATCH_C_WORDS + REP_C_COVERED];
        ms.flagged = (int64_t)cw[MATCH_C_WORDS + REP_C_FLAGGED];
        *count_out = ms.spans;
    }
    ms.readbacks = g_readbacks - rb0;
    g_last_match_stats = ms;
    return SA_AMD_OK;
}

// host buffers: the query goes up, ML / POS (4 m bytes each, either may be nullptr) or the first `capacity` spans come back.
// The index's device is current (the caller's guard).
static int match_host(const sa_amd_index &ix, const uint8_t *Q, int32_t m, int32_t C, bool spans, uint32_t *ML, uint32_t *POS, uint32_t *out_spans,
                      int64_t capacity, int64_t *count_out)
{
    if (m < 0 || C < 1 || (m > 0 && !Q)) return SA_AMD_EINVAL;
    if (spans && (capacity < 0 || !count_out || (capacity > 0 && !out_spans))) return SA_AMD_EINVAL;
    const size_t wb = match_layout(m).bytes, qb = align_up((size_t)m + 16, 256), ab = align_up(((size_t)m + 1) * 4, 256);
    CappedRows rows;
    if (spans) rows = CappedRows(capacity, repeat_spans_bound(m, C));
    PooledScope sc(-1, true);
    sc.acquire(wb + qb + (spans ? align_up(rows.bytes(), 256) : 2 * ab));
    void *dW = sc.take(wb);
    uint8_t *dQ = (uint8_t *)sc.take(qb);
    uint32_t *dOut = (uint32_t *)sc.take(spans ? rows.bytes() : ab), *dOut2 = spans ? nullptr : (uint32_t *)sc.take(ab);
    if (sc.rc == SA_AMD_OK && m > 0) sc.rc = hip_status(hipMemcpyAsync(dQ, Q, (size_t)m, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK)
        sc.rc = match_device(ix, dQ, m, C, spans, !spans && ML ? dOut : nullptr, !spans && POS ? dOut2 : nullptr, spans && rows.cap > 0 ? dOut : nullptr,
                             rows.cap, &rows.count, dW, (int64_t)wb, sc.st);
    if (spans) return rows.finish(sc, out_spans, dOut, count_out);
    if (m > 0 && ML) sc.down(ML, dOut, (size_t)m * 4);
    if (m > 0 && POS) sc.down(POS, dOut2, (size_t)m * 4);
    return sc.finish();
}

}  // namespace sa
