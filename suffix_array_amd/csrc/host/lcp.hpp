// host/lcp.hpp -- LCP array from a device-resident text and suffix array (kernels/lcp.hpp): work-block
// layout, the device entry point's sequence and the host-pointer routes.
#pragma once
#include "pipeline.hpp"
#include "host_path.hpp"
#include "scope.hpp"
#include "index.hpp"
#include "../kernels/lcp.hpp"

namespace sa {

static thread_local sa_amd_lcp_stats g_last_lcp_stats;
static thread_local int32_t g_lcp_cap = -1;         // sa_amd_lcp_set_compare_cap of the calling thread (-1: LCP_CAP_DEFAULT)

// layout of the work block: error + control words | Φ / v / PLCP | four n-entry buffers (binned scatter's pairs, then the long
// lists and their mismatch words) | sort spine | single-pass granules | tile maxima.  Never more than the streaming integrity
// check's block (the rank array there is Φ here; the tile maxima are smaller than its first-byte bitmap).
struct LcpLayout { size_t ctl, phi, alt, alt_elems, spine, status, tiles, bytes; };
static LcpLayout lcp_layout(int32_t n)
{
    LcpLayout L;
    const size_t N1 = (size_t)n + 1;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = align_up(off + b, 256); return o; };
    L.ctl = take(256);                     // bytes 0..15: the sort scratch's error words; 32: range flags; 64..: LCP_C_* (uint64)
    L.phi = take(N1 * 4);
    L.alt_elems = (N1 + 67) & ~(size_t)3;
    L.alt = take(4 * L.alt_elems * 4);
    L.spine = take(SortScratch::SPINE_BYTES);
    L.status = take(SortScratch::granule_bytes((int64_t)N1));
    L.tiles = take(((size_t)ceil_div((int64_t)N1, LCP_TILE) + 1) * 4);
    L.bytes = off;
    return L;
}

constexpr int LCP_CTL_OFF = 64;            // byte offset of the control words in the ctl slab
constexpr int LCP_FLAGS_WORD = 8;          // uint32 index of the range pass's flags in the ctl slab
constexpr int LCP_MAX_ROUNDS = 64;         // doubling windows from 16 bytes cover 2^31 in fewer than 32

// The range pass every entry point starts with, before anything reads through the entries: the control slab is cleared, an
// entry > n is SA_AMD_ERANGE, SA[0] != n (or n in another slot) SA_AMD_EINVAL.
static int lcp_range(const uint32_t *dSA, int64_t n, void *dWork, const LcpLayout &L, hipStream_t st)
{
    uint32_t *err = (uint32_t *)((char *)dWork + L.ctl);
    HIP_TRY(hipMemsetAsync(err, 0, 256, st));
    int64_t blocks = ceil_div(n + 1, 256);
    if (blocks > 16384) blocks = 16384;
    PROF(KC_LCP_PHI, n + 1, st, hipLaunchKernelGGL(k_ci_range, dim3((unsigned)blocks), dim3(256), 0, st, dSA, n, err + LCP_FLAGS_WORD));
    uint32_t f = 0;
    const int rcw = read_words(&f, err + LCP_FLAGS_WORD, 4, st); if (rcw) return rcw;
    if (f & 1u) return SA_AMD_ERANGE;
    if (f & 2u) return SA_AMD_EINVAL;                 // SA[0] != n (or n in another slot)
    return SA_AMD_OK;
}

// Partner-array stage of the LCP array: Φ[SA[i]] = SA[i-1] into the Φ buffer (n > 0, behind lcp_range).
static int lcp_partner_phi(const uint32_t *dSA, int64_t n, void *dWork, const LcpLayout &L, hipStream_t st, const Tuning &tn)
{
    char *base = (char *)dWork;
    uint32_t *err = (uint32_t *)(base + L.ctl);
    uint32_t *phi = (uint32_t *)(base + L.phi);
    uint32_t *alt = (uint32_t *)(base + L.alt);
    const size_t ae = L.alt_elems;
    if (binned(n, n, tn)) {
        // the binned scatter of the ISA writes, keyed by SA[i] with the value SA[i-1]: the sort passes move the pairs, so they
        // are copies (the caller's array is read-only)
        const SortScratch ss = SortScratch::make(base + L.spine, base + L.status, err);
        HIP_TRY(hipMemcpyAsync(alt, dSA + 1, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(alt + ae, dSA, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        sa_amd_stats local;
        memset(&local, 0, sizeof(local));
        const int rcs = scatter_binned(ss, phi, alt, alt + ae, alt + 2 * ae, alt + 3 * ae, n, n, st, &local, tn);
        if (rcs) return rcs;
    } else {
        int64_t pb = ceil_div(n, 256);
        if (pb > 16384) pb = 16384;
        PROF(KC_LCP_PHI, n, st, hipLaunchKernelGGL(k_lcp_phi, dim3((unsigned)pb), dim3(256), 0, st, dSA, n, phi));
    }

    return SA_AMD_OK;
}

// Value stage: phi (n entries, 16-byte aligned) holds ANY partner array in text order, every entry <= n or clamped to n (n: no
// partner, value 0).  Position j is compared directly unless j > 0, phi[j] is neither 0 nor n and T[j-1] == T[phi[j]-1]; for
// the partner arrays this is used with (Φ of the LCP array; the nearest smaller suffix-array neighbours of host/lz.hpp) such a
// position's value is its predecessor's minus one and j + value never decreases, so the max-scan fills it in.  Afterwards
// phi[j] = lcp(T[j..], T[partner[j]..]), the four n-entry buffers are free and the control slab holds the LCP_C_* words; nothing
// has been synchronised since the last read-back.  stats: irreducible, compared_bytes and long_pairs are SET from the
// control words (the caller clears LCP_C_* between two runs over one work block and sums).
static int lcp_values(const uint8_t *dT, int64_t n, uint32_t *phi, void *dWork, const LcpLayout &L, hipStream_t st, sa_amd_lcp_stats &stats)
{
    char *base = (char *)dWork;
    uint32_t *err = (uint32_t *)(base + L.ctl);
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl + LCP_CTL_OFF);
    uint32_t *alt = (uint32_t *)(base + L.alt);
    const size_t ae = L.alt_elems;

    // ---- irreducible values up to the cap; the rest to the long list ----
    const int64_t tiles = ceil_div(n, LCP_TILE);
    const int64_t cap = g_lcp_cap < 0 ? LCP_CAP_DEFAULT : g_lcp_cap;
    uint32_t *tile_max = (uint32_t *)(base + L.tiles);
    uint32_t *list = alt, *res = alt + ae, *list2 = alt + 2 * ae, *res2 = alt + 3 * ae;
    PROF(KC_LCP_IRRED, n, st, hipLaunchKernelGGL(k_lcp_irreducible, dim3((unsigned)tiles), dim3(LCP_THREADS), 0, st, dT, n, phi, cap,
                                                 list, res, tile_max, ctl));
    uint32_t head[(LCP_CTL_OFF + LCP_C_WORDS * 8) / 4];
    { const int rcw = read_words(head, err, sizeof(head), st); if (rcw) return rcw; }
    if (head[0]) return SA_AMD_EINTERNAL;           // a look-back of the binned scatter's sort gave up (never seen; never a silent wrong Φ)
    unsigned long long cw[LCP_C_WORDS];
    memcpy(cw, (const char *)head + LCP_CTL_OFF, sizeof(cw));
    int64_t cnt = (int64_t)cw[LCP_C_LONG];
    stats.irreducible = (int64_t)cw[LCP_C_IRRED];
    stats.compared_bytes = (int64_t)cw[LCP_C_BYTES];
    stats.long_pairs = cnt;

    // ---- long compares: windows that double, every pair of the list spread over the whole GPU ----
    int64_t lo = cap, win = cap > LCP_PIECE ? cap : LCP_PIECE;
    for (int round = 0; cnt > 0; ++round) {
        if (round >= LCP_MAX_ROUNDS) return SA_AMD_EINTERNAL;
        HIP_TRY(hipMemsetAsync(&ctl[LCP_C_NEXT], 0, 8, st));
        const int64_t units = cnt * ceil_div(win, LCP_PIECE);
        int64_t gb = ceil_div(units, LCP_THREADS);
        if (gb > 65536) gb = 65536;
        PROF(KC_LCP_LONG, units * LCP_PIECE, st, hipLaunchKernelGGL(k_lcp_long, dim3((unsigned)gb), dim3(LCP_THREADS), 0, st, dT, n,
                                                                    (const uint32_t *)phi, (const uint32_t *)list, cnt, lo, win, res, ctl));
        int64_t sb = ceil_div(cnt, LCP_THREADS);
        if (sb > 16384) sb = 16384;
        PROF(KC_LCP_LONG, cnt, st, hipLaunchKernelGGL(k_lcp_settle, dim3((unsigned)sb), dim3(LCP_THREADS), 0, st, n, phi,
                                                      (const uint32_t *)list, (const uint32_t *)res, cnt, lo + win, list2, res2, tile_max, ctl));
        { const int rcw = read_words(cw, ctl, sizeof(cw), st); if (rcw) return rcw; }
        cnt = (int64_t)cw[LCP_C_NEXT];
        stats.compared_bytes = (int64_t)cw[LCP_C_BYTES];
        std::swap(list, list2);
        std::swap(res, res2);
        lo += win;
        win *= 2;
    }

    // ---- PLCP[j] = max(v[0..j]) - j ----
    PROF(KC_LCP_SCAN, tiles, st, hipLaunchKernelGGL(k_lcp_scan_spine, dim3(1), dim3(LCP_SPINE_THREADS), 0, st, tile_max, tiles));
    PROF(KC_LCP_SCAN, n, st, hipLaunchKernelGGL(k_lcp_scan, dim3((unsigned)tiles), dim3(LCP_THREADS), 0, st, phi, n, (const uint32_t *)tile_max));
    return SA_AMD_OK;
}

// The stages both the LCP array and the repeat finder (host/repeats.hpp) start with: the range pass, Φ, and the value stage over
// it.  Afterwards PLCP stands in text order in the Φ buffer (n entries), the four n-entry buffers are free and the control slab
// holds the LCP_C_* words; nothing has been synchronised since the last read-back.
// n == 0: returns behind the range pass.  dWork: lcp_layout(n).bytes (L), 256-byte aligned; stats: irreducible, compared_bytes
// and long_pairs are filled in.
static int lcp_front(const uint8_t *dT, const uint32_t *dSA, int64_t n, void *dWork, const LcpLayout &L, hipStream_t st, const Tuning &tn,
                     sa_amd_lcp_stats &stats)
{
    { const int rcr = lcp_range(dSA, n, dWork, L, st); if (rcr) return rcr; }
    if (n == 0) return SA_AMD_OK;
    { const int rcp = lcp_partner_phi(dSA, n, dWork, L, st, tn); if (rcp) return rcp; }
    return lcp_values(dT, n, (uint32_t *)((char *)dWork + L.phi), dWork, L, st, stats);
}

// dT, dSA (n + 1 entries, SA[0] = n), dLCP (n + 1 entries): device memory on the current device; dWork: lcp_layout(n).bytes,
// 256-byte aligned.  Blocks until the array is complete.
static int lcp_device(const uint8_t *dT, const uint32_t *dSA, int32_t n32, uint32_t *dLCP, void *dWork, int64_t work_bytes, hipStream_t st)
{
    const int64_t n = n32;
    sa_amd_lcp_stats stats;
    memset(&stats, 0, sizeof(stats));
    g_last_lcp_stats = stats;
    const LcpLayout L = lcp_layout(n32);
    if (work_bytes < (int64_t)L.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    const Tuning tn = route_tuning();
    const int rb0 = g_readbacks;
    { const int rcf = lcp_front(dT, dSA, n, dWork, L, st, tn, stats); if (rcf) return rcf; }
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(dLCP, 0, 4, st));
        HIP_TRY(hipStreamSynchronize(st));
        stats.readbacks = g_readbacks - rb0;
        g_last_lcp_stats = stats;
        return SA_AMD_OK;
    }

    // ---- LCP[i] = PLCP[SA[i]] ----
    const uint32_t *plcp = (const uint32_t *)((char *)dWork + L.phi);
    int64_t gb = ceil_div(n + 1, 256 * 4);
    if (gb > 65536) gb = 65536;
    PROF(KC_LCP_GATHER, n + 1, st, hipLaunchKernelGGL(k_lcp_gather, dim3((unsigned)gb), dim3(256), 0, st, dSA, n, plcp, dLCP));
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    stats.readbacks = g_readbacks - rb0;
    g_last_lcp_stats = stats;
    return SA_AMD_OK;
}

// host buffers: the text and the suffix array go up (with_build: the array is built on the device instead and comes back
// together with the LCP array), the LCP array comes back.
static int lcp_host(const uint8_t *T, int32_t n, uint32_t *SA, uint32_t *LCP, bool with_build)
{
    if (n < 0 || !SA || !LCP || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    const size_t N1 = (size_t)n + 1;
    PooledScope sc(pick_device(), true);
    const Inputs in = upload_inputs(sc, T, n, with_build ? nullptr : SA, lcp_layout(n).bytes, align_up(N1 * 4, 256));
    uint32_t *dL = (uint32_t *)sc.take(N1 * 4);
    if (sc.rc == SA_AMD_OK) sc.rc = lcp_device(in.dT, in.dSA, n, dL, in.dW, (int64_t)in.wb, sc.st);
    if (with_build) sc.down(SA, in.dSA, N1 * 4);
    sc.down(LCP, dL, N1 * 4);
    return sc.finish();
}

// the index's resident text and array: only the work block and the output come from the pool; on the null stream
static int32_t lcp_index(const sa_amd_index &ix, uint32_t *LCP)
{
    const size_t lb = ((size_t)ix.n + 1) * 4;
    PooledScope sc(ix.device, false);
    const Inputs in = resident_inputs(sc, ix.text(), ix.sa(), lcp_layout(ix.n).bytes, lb);
    uint32_t *dL = (uint32_t *)sc.take(lb);
    if (sc.rc == SA_AMD_OK) sc.rc = lcp_device(in.dT, in.dSA, ix.n, dL, in.dW, (int64_t)in.wb, sc.st);
    sc.down(LCP, dL, lb);
    return sc.finish();
}

}  // namespace sa
