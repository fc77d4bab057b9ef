// host/bwt.hpp -- Burrows-Wheeler transform and its inverse on device-resident data (kernels/bwt.hpp):
// work-block layouts, the two device entry points' sequences and the host-pointer routes.
#pragma once
#include "pipeline.hpp"
#include "host_path.hpp"
#include "scope.hpp"
#include "index.hpp"
#include "../kernels/bwt.hpp"

namespace sa {

static thread_local sa_amd_unbwt_stats g_last_unbwt_stats;
static thread_local int32_t g_unbwt_cap = -1;            // sa_amd_unbwt_set_walk_limits of the calling thread (-1: UNBWT_CAP_DEFAULT)
static thread_local int32_t g_unbwt_spacing = -1;        // sa_amd_unbwt_set_splitter_spacing of the calling thread (-1: UNBWT_SPACING_DEFAULT)
static thread_local int32_t g_unbwt_launches = -1;       // (-1: as many launches as UNBWT_RESTART_WALKS * S steps take)

constexpr size_t BWT_WORK_BYTES = 256;                   // forward: the control slab only
constexpr int UNBWT_CTL_OFF = 64;                        // byte offset of the uint64 counters in the control slab

// ---------------------------------------------------------------- forward ----

// dT (n bytes, any byte address), dSA (n + 1 entries), dB (n bytes, not dT): device memory on the current device; dWork: 256 bytes,
// 256-byte aligned.  Blocks until B is complete.
static int bwt_device(const uint8_t *dT, const uint32_t *dSA, int32_t n32, uint8_t *dB, int32_t *primary_out, void *dWork,
                      int64_t work_bytes, hipStream_t st)
{
    const int64_t n = n32;
    if (work_bytes < (int64_t)BWT_WORK_BYTES || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    if (n > 0 && (const uint8_t *)dB == dT) return SA_AMD_EINVAL;
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    uint32_t *ctl = (uint32_t *)dWork;
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));

    // ---- range pass before anything reads through the entries ----
    int64_t blocks = ceil_div(n + 1, BWT_THREADS);
    if (blocks > 16384) blocks = 16384;
    PROF(KC_BWT_GATHER, n + 1, st, hipLaunchKernelGGL(k_bwt_range, dim3((unsigned)blocks), dim3(BWT_THREADS), 0, st, dSA, n, ctl));
    uint32_t w[4] = { 0, 0, 0, 0 };
    { const int rcw = read_words(w, ctl + BWT_W_FLAGS, sizeof(w), st); if (rcw) return rcw; }
    if (w[0] & 1u) return SA_AMD_ERANGE;
    if (w[0] & 2u) return SA_AMD_EINVAL;                  // SA[0] != n (or n in another slot)
    if (n == 0) { *primary_out = 0; return SA_AMD_OK; }
    if (w[1] != 1u) return SA_AMD_EINVAL;                 // not exactly one entry equal to 0
    const int64_t primary = w[2];

    int64_t gb = ceil_div(ceil_div(n, 4), BWT_THREADS);
    if (gb > 65536) gb = 65536;
    PROF(KC_BWT_GATHER, n, st, hipLaunchKernelGGL(k_bwt_gather, dim3((unsigned)gb), dim3(BWT_THREADS), 0, st, dT, dSA, n, primary, dB,
                                                  (((uintptr_t)dSA) & 15u) == 0 ? 1 : 0, (((uintptr_t)dB) & 3u) == 0 ? 1 : 0));
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    *primary_out = (int32_t)primary;
    return SA_AMD_OK;
}

// The transform of a resident text and array into a slab of the scope's block; n bytes and `primary` come back.  in.dW: the
// scope's first slab, at least BWT_WORK_BYTES.
static int bwt_resident(PooledScope &sc, const Inputs &in, int32_t n, uint8_t *B, int32_t *primary_out)
{
    uint8_t *dB = (uint8_t *)sc.take((size_t)n + 16);
    if (sc.rc == SA_AMD_OK) sc.rc = bwt_device(in.dT, in.dSA, n, dB, primary_out, in.dW, (int64_t)in.wb, sc.st);
    if (n > 0) sc.down(B, dB, (size_t)n);
    return sc.finish();
}

// host buffers: the text goes up; the array is built on the device and stays there (SA == nullptr) or the caller's goes up
static int bwt_host(const uint8_t *T, int32_t n, const uint32_t *SA, uint8_t *B, int32_t *primary_out)
{
    if (n < 0 || !primary_out || (n > 0 && (!T || !B))) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    PooledScope sc(pick_device(), true);
    const Inputs in = upload_inputs(sc, T, n, SA, BWT_WORK_BYTES, align_up((size_t)n + 16, 256));
    return bwt_resident(sc, in, n, B, primary_out);
}

// ---------------------------------------------------------------- inverse ----

// layout of the work block: error + control words | digit starts | ψ | one (n + 1)-entry buffer (the sorted keys, then the
// row -> walker index) | two more (the keys and the sort's values, then the walker tables: five words per walker) | sort spine |
// single-pass granules.  About 16.5 bytes per byte of text: less than the LCP array's block.
struct UnbwtLayout { size_t ctl, starts, psi, widx, wk, alt_elems, spine, status, bytes; };
static UnbwtLayout unbwt_layout(int32_t n)
{
    UnbwtLayout L;
    const size_t N1 = (size_t)n + 1;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = align_up(off + b, 256); return o; };
    L.ctl = take(256);                     // bytes 0..15: the sort scratch's error words; 32..: UNBWT_W_* (uint32); 64..: UNBWT_C_* (uint64)
    L.starts = take(257 * 4);
    L.psi = take(N1 * 4);
    L.alt_elems = (N1 + 67) & ~(size_t)3;
    L.widx = take(L.alt_elems * 4);
    L.wk = take(2 * L.alt_elems * 4);
    L.spine = take(SortScratch::SPINE_BYTES);
    L.status = take(SortScratch::granule_bytes((int64_t)N1));
    L.bytes = off;
    return L;
}

// dB (n bytes, any byte address), dT_out (n bytes): device memory on the current device; dWork: unbwt_layout(n).bytes, 256-byte
// aligned.  Blocks until the text is complete.  SA_AMD_EINVAL, with nothing written to dT_out, when (B, primary) is not the
// transform of any text.
static int unbwt_device(const uint8_t *dB, int32_t n32, int32_t primary32, uint8_t *dT_out, void *dWork, int64_t work_bytes, hipStream_t st)
{
    const int64_t n = n32;
    sa_amd_unbwt_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_unbwt_stats = stats;
    if (n == 0) return primary32 == 0 ? SA_AMD_OK : SA_AMD_EINVAL;
    if (primary32 < 1 || primary32 > n32) return SA_AMD_EINVAL;
    const UnbwtLayout L = unbwt_layout(n32);
    if (work_bytes < (int64_t)L.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    const Tuning tn = route_tuning();
    const int rb0 = g_readbacks;
    const uint32_t primary = (uint32_t)primary32;
    char *base = (char *)dWork;
    uint32_t *ctl = (uint32_t *)(base + L.ctl);
    unsigned long long *ctl64 = (unsigned long long *)(base + L.ctl + UNBWT_CTL_OFF);
    uint32_t *starts = (uint32_t *)(base + L.starts), *psi = (uint32_t *)(base + L.psi);
    uint32_t *widx = (uint32_t *)(base + L.widx), *wk = (uint32_t *)(base + L.wk);
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));

    // ---- phase 1: ψ by one stable digit sort of the indices of B ----
    {
        const SortScratch ss = SortScratch::make(base + L.spine, base + L.status, ctl);
        uint32_t *keys = wk, *altv = wk + L.alt_elems, *altk = widx;
        int64_t gb = ceil_div(ceil_div(n, 4), BWT_THREADS);
        if (gb > 65536) gb = 65536;
        PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_unbwt_keys, dim3((unsigned)gb), dim3(BWT_THREADS), 0, st, dB, n, keys,
                                                (((uintptr_t)dB) & 3u) == 0 ? 1 : 0));
        SortJob<uint32_t> job{ keys, nullptr, altk, altv, n, 0, RADIX_BITS };
        job.iota = true;
        SortResult<uint32_t> pr;
        const int rcs = sort_pairs32(job, ss, st, tn, &pr);
        if (rcs) return rcs;
        if (pr.passes > 1) return SA_AMD_EINTERNAL;
        int64_t pb = ceil_div(n, BWT_THREADS);
        if (pb > 16384) pb = 16384;
        PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_unbwt_psi, dim3((unsigned)pb), dim3(BWT_THREADS), 0, st, (const uint32_t *)pr.keys,
                                                (const uint32_t *)(pr.passes ? pr.vals : nullptr), n, primary, psi, starts));
    }

    // ---- phase 2: every splitter walks to the next one; denser splitters when walks are still going after the launch limit ----
    const int64_t mcap = (int64_t)((2 * L.alt_elems) / 5) & ~(int64_t)1;
    uint32_t *srow = wk;
    unsigned long long *P0 = (unsigned long long *)(wk + mcap), *P1 = (unsigned long long *)(wk + 3 * mcap);
    const int64_t cap = g_unbwt_cap < 0 ? UNBWT_CAP_DEFAULT : g_unbwt_cap;
    int64_t S = g_unbwt_spacing < 0 ? UNBWT_SPACING_DEFAULT : g_unbwt_spacing;
    uint32_t seed = 0;
    int64_t m = 0, longest = 0;
    uint32_t pidx = 0;
    for (;; ++seed) {
        const bool last_try = S <= UNBWT_SPACING_MIN;
        HIP_TRY(hipMemsetAsync(ctl + UNBWT_W_M, 0, 256 - UNBWT_W_M * 4, st));
        int64_t sb = ceil_div(n + 1, BWT_THREADS);
        if (sb > 16384) sb = 16384;
        PROF(KC_UNBWT_WALK, n + 1, st, hipLaunchKernelGGL(k_unbwt_splitters, dim3((unsigned)sb), dim3(BWT_THREADS), 0, st, n + 1, primary,
                                                          (uint32_t)(S - 1), seed, srow, widx, (uint32_t)mcap, ctl));
        uint32_t head[UNBWT_W_PIDX + 1];
        { const int rcw = read_words(head, ctl, sizeof(head), st); if (rcw) return rcw; }
        if (head[0]) return SA_AMD_EINTERNAL;            // a look-back of the sort gave up (never seen; never a silent wrong ψ)
        m = head[UNBWT_W_M];
        pidx = head[UNBWT_W_PIDX];
        if (m < 1 || m > mcap || (int64_t)pidx >= m) return SA_AMD_EINTERNAL;
        const int64_t limit = g_unbwt_launches > 0 ? g_unbwt_launches : ceil_div(UNBWT_RESTART_WALKS * S, cap);
        const unsigned wgrid = (unsigned)ceil_div(m, BWT_THREADS);
        unsigned long long cw[UNBWT_C_WORDS] = { 1, 0, 0 };
        int64_t launches = 0;
        while (cw[UNBWT_C_ACTIVE] != 0 && (last_try || launches < limit)) {
            HIP_TRY(hipMemsetAsync(&ctl64[UNBWT_C_ACTIVE], 0, 8, st));
            PROF(KC_UNBWT_WALK, m, st, hipLaunchKernelGGL(k_unbwt_walk, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const uint32_t *)psi, primary,
                                                          (uint32_t)(S - 1), seed, (const uint32_t *)srow, (const uint32_t *)widx, P0, P1, m, cap,
                                                          launches == 0 ? 1 : 0, ctl64));
            { const int rcw = read_words(cw, ctl64, sizeof(cw), st); if (rcw) return rcw; }
            ++launches;
        }
        stats.walk_launches += (int32_t)launches;
        stats.steps += (int64_t)cw[UNBWT_C_STEPS];
        if (cw[UNBWT_C_ACTIVE] == 0) { longest = (int64_t)cw[UNBWT_C_LONGEST]; break; }
        ++stats.restarts;
        S = S / 8 < UNBWT_SPACING_MIN ? UNBWT_SPACING_MIN : S / 8;
    }
    stats.walkers = m;
    stats.splitter_spacing = (int32_t)S;
    stats.longest_walk = longest;

    // ---- rank the m sublists from primary's: pointer jumping, ceil(log2 m) rounds ----
    const unsigned wgrid = (unsigned)ceil_div(m, BWT_THREADS);
    unsigned long long *pin = P0, *pout = P1;
    for (int r = 0; r < bit_length((uint64_t)(m - 1)); ++r) {
        PROF(KC_UNBWT_RANK, m, st, hipLaunchKernelGGL(k_unbwt_rank, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const unsigned long long *)pin, pout, m));
        std::swap(pin, pout);
    }
    uint32_t *wbase = (uint32_t *)pout;
    PROF(KC_UNBWT_RANK, m, st, hipLaunchKernelGGL(k_unbwt_base, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const unsigned long long *)pin, m, pidx, wbase, ctl));
    uint32_t tot[2];
    { const int rcw = read_words(tot, ctl + UNBWT_W_TOTAL, sizeof(tot), st); if (rcw) return rcw; }
    stats.readbacks = g_readbacks - rb0;
    g_last_unbwt_stats = stats;
    if ((int64_t)tot[0] != n + 1 || tot[1] != UNBWT_NIL) return SA_AMD_EINVAL;      // the walk from primary closes early: not a transform

    // ---- phase 3: walk again and write ----
    HIP_TRY(hipMemsetAsync(&ctl64[UNBWT_C_STEPS], 0, 8, st));
    for (int64_t done = 0; done < longest; done += cap)
        PROF(KC_UNBWT_WRITE, m, st, hipLaunchKernelGGL(k_unbwt_write, dim3(wgrid), dim3(BWT_THREADS), 0, st, (const uint32_t *)psi, primary,
                                                       (uint32_t)(S - 1), seed, srow, wbase, m, n, (const uint32_t *)starts, dT_out, cap, ctl64));
    unsigned long long wsteps = 0;
    { const int rcw = read_words(&wsteps, &ctl64[UNBWT_C_STEPS], 8, st); if (rcw) return rcw; }
    g_prof.resolve();
    stats.steps += (int64_t)wsteps;
    stats.readbacks = g_readbacks - rb0;
    g_last_unbwt_stats = stats;
    return SA_AMD_OK;
}

// host buffers: B goes up, the text comes back
static int unbwt_host(const uint8_t *B, int32_t n, int32_t primary, uint8_t *T_out)
{
    if (n < 0 || (n > 0 && (!B || !T_out))) return SA_AMD_EINVAL;
    if (n == 0 ? primary != 0 : (primary < 1 || primary > n)) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    const size_t tb = align_up((size_t)n + 16, 256), wb = unbwt_layout(n).bytes;
    PooledScope sc(pick_device(), true);
    sc.acquire(wb + 2 * tb);
    void *dW = sc.take(wb);
    uint8_t *dB = (uint8_t *)sc.take(tb), *dT = (uint8_t *)sc.take(tb);
    if (sc.rc == SA_AMD_OK && n > 0) sc.rc = hip_status(hipMemcpyAsync(dB, B, (size_t)n, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK) sc.rc = unbwt_device(dB, n, primary, dT, dW, (int64_t)wb, sc.st);
    if (n > 0) sc.down(T_out, dT, (size_t)n);
    return sc.finish();
}

// the index's resident text and array: only the work block and the output come from the pool; on the null stream
static int32_t bwt_index(const sa_amd_index &ix, uint8_t *BWT, int32_t *primary_out)
{
    PooledScope sc(ix.device, false);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), BWT_WORK_BYTES, (size_t)ix.n + 16);
    return bwt_resident(sc, in, ix.n, BWT, primary_out);
}

}  // namespace sa
