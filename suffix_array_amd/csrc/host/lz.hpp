// host/lz.hpp -- Lempel-Ziv factorisation from a device-resident text and suffix array (kernels/lz.hpp):
// work-block layout, the device entry point's sequence and the host-pointer routes.
#pragma once
#include "lcp.hpp"
#include "bwt.hpp"
#include "repeats.hpp"
#include "../kernels/lz.hpp"

namespace sa {

static thread_local sa_amd_lz_stats g_last_lz_stats;

constexpr int LZ_CTL_OFF = 128;            // byte offset of the LZ_C_* words in the LCP control slab (behind the LCP_C_* words)
static_assert(LCP_CTL_OFF + LCP_C_WORDS * 8 <= LZ_CTL_OFF && LZ_CTL_OFF + LZ_C_WORDS * 8 <= 256, "control slab");
static_assert(UNBWT_CTL_OFF + UNBWT_C_WORDS * 8 <= LZ_CTL_OFF && (UNBWT_W_TAIL + 1) * 4 <= UNBWT_CTL_OFF, "the walk's words lie in front");

// layout of the work block: the LCP array's block | three n-entry buffers.  Stage 1: the slot arrays and the levels in the LCP
// block's n-entry buffers, P in the Φ buffer, N in the first extra buffer, their copies in the other two.  Value stages: lp over
// P, ln over N, the long lists in the LCP block's buffers both times.  Parse: LPF, SRC, the splitter list and a pointer table
// in the LCP block's buffers, position -> walker in the Φ buffer, the second pointer table, the walkers' places (then the
// marks) in the extra buffers; at the end the flag bytes over the first pointer table and the tile counts over the second.
struct LzLayout { LcpLayout lcp; size_t xs, bytes; };
static LzLayout lz_layout(int32_t n)
{
    LzLayout Z;
    Z.lcp = lcp_layout(n);
    Z.xs = Z.lcp.bytes;
    Z.bytes = Z.xs + align_up(3 * Z.lcp.alt_elems * 4, 256);
    return Z;
}

static LzLevels lz_levels(int64_t n, uint32_t *base)
{
    LzLevels lv;
    memset(&lv, 0, sizeof(lv));
    lv.base = base;
    int64_t off = 0, span = LZ_FAN;
    for (int k = 1; k < LZ_MAX_LEVELS; ++k, span *= LZ_FAN) {
        lv.cnt[k] = ceil_div(n, span);
        lv.off[k] = off;
        off += lv.cnt[k];
        lv.top = k;
        if (k >= 2 && lv.cnt[k] <= LZ_FAN) break;
    }
    return lv;
}

// Stage 1 over A[0 .. n) (n > 0): psl, nsl n entries each, levels n / 31 + 8 words.  Pphi != nullptr: the two partner arrays
// in text order (every A[i] < n is written through); else the finished neighbour slots stay in psl / nsl.
// LEQ_LEFT (values below 2^31, the slots stay): the left neighbour is the nearest value <= A[i] (host/substrings.hpp).
template <bool LEQ_LEFT = false>
static int lz_nsv(const uint32_t *A, int64_t n, uint32_t *psl, uint32_t *nsl, uint32_t *levels, uint32_t *Pphi, uint32_t *Nphi,
                  unsigned long long *ctl, hipStream_t st)
{
    const LzLevels lv = lz_levels(n, levels);
    const int64_t tiles = ceil_div(n, LZ_TILE);
    PROF(KC_LCP_PHI, n, st, hipLaunchKernelGGL((k_lz_tile<LEQ_LEFT>), dim3((unsigned)tiles), dim3(LZ_THREADS), 0, st, A, n, psl, nsl, levels + lv.off[1],
                                               levels + lv.off[2], ctl));
    for (int k = 3; k <= lv.top; ++k)
        PROF(KC_LCP_PHI, lv.cnt[k], st, hipLaunchKernelGGL(k_lz_level, dim3((unsigned)ceil_div(lv.cnt[k], LZ_THREADS)), dim3(LZ_THREADS), 0, st,
                                                           (const uint32_t *)(levels + lv.off[k - 1]), lv.cnt[k - 1], levels + lv.off[k], lv.cnt[k]));
    const unsigned g = (unsigned)ceil_div(n, LZ_THREADS);
    if (LEQ_LEFT) PROF(KC_LCP_PHI, n, st, hipLaunchKernelGGL((k_lz_far<false, true>), dim3(g), dim3(LZ_THREADS), 0, st, A, n, psl, nsl, lv, Pphi, Nphi, ctl));
    else if (Pphi) PROF(KC_LCP_PHI, n, st, hipLaunchKernelGGL((k_lz_far<true>), dim3(g), dim3(LZ_THREADS), 0, st, A, n, psl, nsl, lv, Pphi, Nphi, ctl));
    else PROF(KC_LCP_PHI, n, st, hipLaunchKernelGGL((k_lz_far<false>), dim3(g), dim3(LZ_THREADS), 0, st, A, n, psl, nsl, lv, Pphi, Nphi, ctl));
    return SA_AMD_OK;
}

// dT, dSA (n + 1 entries, SA[0] = n): device memory on the current device; dWork: lz_layout(n).bytes, 256-byte aligned.
// !parse: LPF and SRC (n entries each, either may be null).  parse: the first `capacity` phrases to dPhrases, the number of all
// of them to *count_out (host).  Blocks until done.
static int lz_device(const uint8_t *dT, const uint32_t *dSA, int32_t n32, bool parse, uint32_t *dLPF, uint32_t *dSRC, uint32_t *dPhrases,
                     int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes, hipStream_t st)
{
    const int64_t n = n32;
    sa_amd_lz_stats zs;
    memset(&zs, 0, sizeof(zs));
    zs.longest_pos = -1;
    g_last_lz_stats = zs;
    sa_amd_lcp_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_lcp_stats = stats;
    const LzLayout Z = lz_layout(n32);
    const LcpLayout &L = Z.lcp;
    if (work_bytes < (int64_t)Z.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    if (parse && (capacity < 0 || !count_out || (capacity > 0 && !dPhrases))) return SA_AMD_EINVAL;
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const int rb0 = g_readbacks;
    { const int rcr = lcp_range(dSA, n, dWork, L, st); if (rcr) return rcr; }
    if (n == 0) {
        if (parse) *count_out = 0;
        zs.readbacks = g_readbacks - rb0;
        g_last_lz_stats = zs;
        return SA_AMD_OK;
    }

    char *base = (char *)dWork;
    uint32_t *ctl32 = (uint32_t *)(base + L.ctl);
    unsigned long long *lcpc = (unsigned long long *)(base + L.ctl + LCP_CTL_OFF);
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl + LZ_CTL_OFF);
    uint32_t *phi = (uint32_t *)(base + L.phi);
    uint32_t *alt = (uint32_t *)(base + L.alt);
    const size_t ae = L.alt_elems;
    uint32_t *x0 = (uint32_t *)(base + Z.xs), *x1 = x0 + ae, *x2 = x0 + 2 * ae;

    // ---- stage 1: P into the Φ buffer, N into x0; copies for the merge (the value stage overwrites its partner array) ----
    { const int rcn = lz_nsv(dSA + 1, n, alt, alt + ae, alt + 2 * ae, phi, x0, ctl, st); if (rcn) return rcn; }
    HIP_TRY(hipMemcpyAsync(x1, phi, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(x2, x0, (size_t)n * 4, hipMemcpyDeviceToDevice, st));

    // ---- lp and ln: the LCP array's value stage, twice ----
    { const int rcv = lcp_values(dT, n, phi, dWork, L, st, stats); if (rcv) return rcv; }
    sa_amd_lcp_stats second;
    memset(&second, 0, sizeof(second));
    HIP_TRY(hipMemsetAsync(lcpc, 0, LCP_C_WORDS * 8, st));
    { const int rcv = lcp_values(dT, n, x0, dWork, L, st, second); if (rcv) return rcv; }
    stats.irreducible += second.irreducible;
    stats.compared_bytes += second.compared_bytes;
    stats.long_pairs += second.long_pairs;

    uint32_t *lpf = parse ? alt : dLPF, *src = parse ? alt + ae : dSRC;
    int64_t mb = ceil_div(n, LZ_THREADS);
    if (mb > 65536) mb = 65536;
    if (lpf || src)
        PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL(k_lz_merge, dim3((unsigned)mb), dim3(LZ_THREADS), 0, st, (const uint32_t *)phi, (const uint32_t *)x0,
                                                     (const uint32_t *)x1, (const uint32_t *)x2, n, lpf, src));

    if (parse) {
        // ---- every splitter walks to the next one; denser splitters when walks are still going after the launch limit ----
        unsigned long long *wc = (unsigned long long *)(base + L.ctl + UNBWT_CTL_OFF);
        uint32_t *widx = phi, *srow = alt + 2 * ae, *J0 = alt + 3 * ae, *J1 = x0;
        unsigned long long *state = (unsigned long long *)x1;
        const int64_t mcap = (int64_t)ae;
        const int64_t cap = g_unbwt_cap < 0 ? UNBWT_CAP_DEFAULT : g_unbwt_cap;
        int64_t S = g_unbwt_spacing < 0 ? UNBWT_SPACING_DEFAULT : g_unbwt_spacing;
        uint32_t seed = 0, pidx = 0;
        int64_t m = 0, longest = 0;
        for (;; ++seed) {
            const bool last_try = S <= UNBWT_SPACING_MIN;
            HIP_TRY(hipMemsetAsync(ctl32 + UNBWT_W_M, 0, LZ_CTL_OFF - UNBWT_W_M * 4, st));
            int64_t sb = ceil_div(n, BWT_THREADS);
            if (sb > 16384) sb = 16384;
            PROF(KC_UNBWT_WALK, n, st, hipLaunchKernelGGL(k_unbwt_splitters, dim3((unsigned)sb), dim3(BWT_THREADS), 0, st, n, 0u, (uint32_t)(S - 1), seed,
                                                          srow, widx, (uint32_t)mcap, ctl32));
            uint32_t head[UNBWT_W_PIDX + 1];
            { const int rcw = read_words(head, ctl32, sizeof(head), st); if (rcw) return rcw; }
            m = head[UNBWT_W_M];
            pidx = head[UNBWT_W_PIDX];
            if (m < 1 || m > mcap || (int64_t)pidx >= m) return SA_AMD_EINTERNAL;
            const int64_t limit = g_unbwt_launches > 0 ? g_unbwt_launches : ceil_div(UNBWT_RESTART_WALKS * S, cap);
            const unsigned wgrid = (unsigned)ceil_div(m, BWT_THREADS);
            unsigned long long cw[UNBWT_C_WORDS] = { 1, 0, 0 };
            int64_t launches = 0;
            while (cw[UNBWT_C_ACTIVE] != 0 && (last_try || launches < limit)) {
                HIP_TRY(hipMemsetAsync(&wc[UNBWT_C_ACTIVE], 0, 8, st));
                PROF(KC_UNBWT_WALK, m, st, hipLaunchKernelGGL(k_lz_walk, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const uint32_t *)lpf, n, (uint32_t)(S - 1),
                                                              seed, (const uint32_t *)srow, (const uint32_t *)widx, J0, state, m, cap,
                                                              launches == 0 ? 1 : 0, wc));
                { const int rcw = read_words(cw, wc, sizeof(cw), st); if (rcw) return rcw; }
                ++launches;
            }
            zs.walk_launches += (int32_t)launches;
            zs.walk_steps += (int64_t)cw[UNBWT_C_STEPS];
            if (cw[UNBWT_C_ACTIVE] == 0) { longest = (int64_t)cw[UNBWT_C_LONGEST]; break; }
            ++zs.restarts;
            S = S / 8 < UNBWT_SPACING_MIN ? UNBWT_SPACING_MIN : S / 8;
        }
        zs.walkers = m;
        zs.splitter_spacing = (int32_t)S;

        // ---- which walkers lie on the path from position 0: marks through pointers that double, ceil(log2 m) rounds ----
        const unsigned wgrid = (unsigned)ceil_div(m, BWT_THREADS);
        uint32_t *mark = (uint32_t *)state;                       // (every walker has arrived: its place is no longer needed)
        HIP_TRY(hipMemsetAsync(mark, 0, (size_t)m * 4, st));
        uint32_t *pin = J0, *pout = J1;
        for (int r = 0; r < bit_length((uint64_t)(m - 1)); ++r) {
            PROF(KC_UNBWT_RANK, m, st, hipLaunchKernelGGL(k_lz_jump, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const uint32_t *)pin, pout, mark, m, pidx));
            std::swap(pin, pout);
        }

        // ---- the walkers on the path flag their positions; flags -> phrases ----
        uint8_t *flag = (uint8_t *)J0;
        uint32_t *cnt = J1;
        HIP_TRY(hipMemsetAsync(flag, 0, (size_t)n, st));
        HIP_TRY(hipMemsetAsync(&wc[UNBWT_C_STEPS], 0, 8, st));
        for (int64_t done = 0; done < longest; done += cap)
            PROF(KC_UNBWT_WRITE, m, st, hipLaunchKernelGGL(k_lz_flag, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const uint32_t *)lpf, n, (uint32_t)(S - 1), seed,
                                                           srow, (const uint32_t *)mark, pidx, m, cap, flag, wc));
        const int64_t tiles = ceil_div(n, REP_TILE);
        PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL((k_lz_emit<0>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, (const uint8_t *)flag,
                                                     (const uint32_t *)lpf, (const uint32_t *)src, n, cnt, dPhrases, capacity, ctl));
        PROF(KC_REP_SPANS, tiles, st, hipLaunchKernelGGL(k_rep_sum_spine, dim3(1), dim3(REP_SPINE_THREADS), 0, st, cnt, tiles, &ctl[LZ_C_PHRASES]));
        PROF(KC_REP_SPANS, n, st, hipLaunchKernelGGL((k_lz_emit<1>), dim3((unsigned)tiles), dim3(REP_THREADS), 0, st, (const uint8_t *)flag,
                                                     (const uint32_t *)lpf, (const uint32_t *)src, n, cnt, dPhrases, capacity, ctl));
    }

    // ---- one read-back: the walk's and the factorisation's counters ----
    uint32_t head[256 / 4];
    { const int rcw = read_words(head, ctl32, sizeof(head), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    unsigned long long cw[LZ_C_WORDS], ww[UNBWT_C_WORDS];
    memcpy(cw, (const char *)head + LZ_CTL_OFF, sizeof(cw));
    memcpy(ww, (const char *)head + UNBWT_CTL_OFF, sizeof(ww));
    zs.unresolved = (int64_t)cw[LZ_C_UNRES];
    zs.hierarchy_steps = (int64_t)cw[LZ_C_HSTEPS];
    zs.hierarchy_max = (int64_t)cw[LZ_C_HMAX];
    if (parse) {
        zs.walk_steps += (int64_t)ww[UNBWT_C_STEPS];
        zs.phrases = (int64_t)cw[LZ_C_PHRASES];
        zs.literals = (int64_t)cw[LZ_C_LITERALS];
        zs.longest = (int64_t)(cw[LZ_C_BEST] >> 32);
        zs.longest_pos = zs.longest > 0 ? (int64_t)(uint32_t)~(uint32_t)cw[LZ_C_BEST] : -1;
        *count_out = zs.phrases;
    }
    zs.readbacks = g_readbacks - rb0;
    g_last_lz_stats = zs;
    stats.readbacks = zs.readbacks;
    g_last_lcp_stats = stats;
    return SA_AMD_OK;
}

// Either form over a resident text and array, the outputs in slabs of the scope's block: LPF and SRC (4 n bytes each, either
// may be null: then the device call gets null and nothing comes back) or the first rows.cap phrases come back.  in.dW: the
// scope's first slab, at least lz_layout(n).bytes.
static int lz_resident(PooledScope &sc, const Inputs &in, int32_t n, bool parse, uint32_t *LPF, uint32_t *SRC, uint32_t *phrases, CappedRows &rows,
                       int64_t *count_out)
{
    const size_t ab = ((size_t)n + 1) * 4;
    uint32_t *dOut = (uint32_t *)sc.take(parse ? rows.bytes() : ab), *dOut2 = parse ? nullptr : (uint32_t *)sc.take(ab);
    if (sc.rc == SA_AMD_OK)
        sc.rc = lz_device(in.dT, in.dSA, n, parse, LPF ? dOut : nullptr, SRC ? dOut2 : nullptr, dOut, rows.cap, &rows.count, in.dW, (int64_t)in.wb, sc.st);
    if (parse) return rows.finish(sc, phrases, dOut, count_out);
    if (n > 0 && LPF) sc.down(LPF, dOut, (size_t)n * 4);
    if (n > 0 && SRC) sc.down(SRC, dOut2, (size_t)n * 4);
    return sc.finish();
}

// host buffers: the text goes up; the array is built on the device and stays there (SA == nullptr) or the caller's goes up
static int lz_host(const uint8_t *T, int32_t n, const uint32_t *SA, bool parse, uint32_t *LPF, uint32_t *SRC, uint32_t *phrases, int64_t capacity,
                   int64_t *count_out)
{
    if (n < 0 || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (parse && (capacity < 0 || !count_out || (capacity > 0 && !phrases))) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    CappedRows rows;
    if (parse) rows = CappedRows(capacity, n);                      // no more phrases than bytes
    PooledScope sc(pick_device(), true);
    const Inputs in = upload_inputs(sc, T, n, SA, lz_layout(n).bytes, parse ? align_up(rows.bytes(), 256) : 2 * align_up(((size_t)n + 1) * 4, 256));
    return lz_resident(sc, in, n, parse, LPF, SRC, phrases, rows, count_out);
}

// the index's resident text and array: only the work block and the outputs come from the pool; on the null stream
static int32_t lz_index(const sa_amd_index &ix, bool parse, uint32_t *LPF, uint32_t *SRC, uint32_t *phrases, int64_t capacity, int64_t *count_out)
{
    if (parse && (capacity < 0 || !count_out || (capacity > 0 && !phrases))) return SA_AMD_EINVAL;
    CappedRows rows;
    if (parse) rows = CappedRows(capacity, ix.n);
    PooledScope sc(ix.device, false);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), lz_layout(ix.n).bytes, parse ? rows.bytes() : 2 * align_up(((size_t)ix.n + 1) * 4, 256));
    return lz_resident(sc, in, ix.n, parse, LPF, SRC, phrases, rows, count_out);
}

}  // namespace sa
