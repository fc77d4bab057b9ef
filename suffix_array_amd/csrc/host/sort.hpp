// host/sort.hpp -- the radix-sort drivers of the device pipeline (host/pipeline.hpp): the single-pass tile scatter's host side
// (sort_pairs, sort_pairs32, sort_first_counts), the in-LDS bucket sort of the 32-bit first stage (bucket_sort32) and, in the
// diagnostic library, the three-kernel pass and the sample sort (sample_sort64).
// Included by host/pipeline.hpp only: the kernels come in through support.hpp and read_words is defined in host/readback.hpp,
// which pipeline.hpp includes behind this file.
#pragma once
#include "support.hpp"
#include "tuning.hpp"

namespace sa {

constexpr int SORT_MAX_WG = 1024;   // spine rows are scanned by one 1024-thread block
// bucket sort of the 32-bit first stage (kernels/bucket_sort.hpp): the top 16 key bits by two global passes of 8 bits (the low 16
// inside the buckets), or the top 18 by two passes of 9 bits (the low 14 inside) for texts whose 16-bit buckets outgrow a workgroup
constexpr int BK_TOP_BITS_MAX = 18;
constexpr uint32_t BK_BUCKETS_MAX = 1u << BK_TOP_BITS_MAX;
static_assert(32 - 16 <= BK_MAX_LBITS, "two 8-bit passes inside a bucket");

#ifdef SA_AMD_DIAG
// (three-kernel pass of rounds 1-2: diagnostic library only, see kernels/radix_sort.hpp)
// Tile-scatter kernel shapes (threads, items per thread, workgroups per CU).  SA_AMD_SORT_VARIANT selects one at run
// time for A/B measurements; every entry of the PRODUCT table sorts correctly.  The diagnostic library appends the
// first-generation scatter, its timing ablations (wrong orders, on purpose) and the phase-stamp build.
typedef void (*DownsweepFn)(const uint64_t *, const uint32_t *, uint64_t *, uint32_t *, uint32_t *,
                            const uint32_t *, int64_t, int, uint32_t, int64_t, int);
struct SortVariant { int threads, items, wg_per_cu; DownsweepFn fn; const char *name; };
static const SortVariant sort_variants[] = {
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8, 16, 1, false, uint64_t, 4>, "carry-completed lines 1024x8 + LDS prefetch of half of the next tile's keys (default)" },
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8>, "carry-completed lines 1024x8" },
    { 512, 16, 1, k_radix_downsweep_wcl<512, 16>, "carry-completed lines 512x16" },
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8, 8>, "carry 1024x8, granule 8" },
    // (two workgroups per CU at 64 VGPRs -- 1024x4 or 512x8 with granule 8 -- measured slower: C3-iid 28.0 -> 29.8 .. 33.9 ms)
#ifdef SA_AMD_DIAG
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4>, "plain tile scatter 1024x8 (first generation)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 1>, "plain 1024x8 ABLATION sequential stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 33>, "plain 1024x8 ABLATION no ranking + sequential stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 16>, "plain 1024x8 ABLATION no stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 49>, "plain 1024x8 ABLATION no ranking, no stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8, 16, 1, true>, "carry 1024x8 DIAGNOSTIC phase stamps (tools/phase_stamps.py)" },
#endif
};
constexpr int N_SORT_VARIANTS = (int)(sizeof(sort_variants) / sizeof(sort_variants[0]));

struct SortGrid { int G; int64_t tiles_per_wg; int tile; };
static SortGrid sort_grid(int64_t count, const SortVariant &sv)
{
    SortGrid g;
    g.tile = sv.threads * sv.items;
    const int64_t tiles = ceil_div(count, g.tile);
    int max_wg = 256 * sv.wg_per_cu;
    if (max_wg > SORT_MAX_WG) max_wg = SORT_MAX_WG;
    g.tiles_per_wg = ceil_div(tiles, max_wg);
    if (g.tiles_per_wg < 1) g.tiles_per_wg = 1;
    g.G = (int)ceil_div(tiles, g.tiles_per_wg);
    if (g.G < 1) g.G = 1;
    return g;
}

#else
constexpr int N_SORT_VARIANTS = 1;      // (the product has one sort engine: the single-pass tile scatter)
#endif

// what a radix sort needs besides its ping-pong buffers
struct SortScratch {
    uint32_t *spine;                // RADIX * SORT_MAX_WG words: per-chunk counts (three-kernel pass) / two zones of segment counts + tickets (single-pass)
    uint32_t *digit_tot;            // RADIX words
    unsigned long long *status;     // single-pass scatter: 256 granules per tile (nullptr: the three-kernel pass is used)
    uint32_t *err;                  // single-pass scatter: look-back give-ups (must stay 0).  A tile whose look-back gave up (2^22 polls without
                                    // an answer: never seen, the bound turns a hang into an error) has scattered with a partial prefix -- in bounds,
                                    // wrong order --, so EVERY user of a SortScratch reads err[0] before it trusts a result: build_device at its end
                                    // (SA_AMD_EINTERNAL), sa_amd_check_integrity_device behind its sorts, the diagnostic hooks behind theirs
};

// ------------------------------------------------------------------------------------------
// Single-pass tile scatter (kernels/onesweep.hpp): host side of one LSD sort.
// Scratch inside the spine slab: ZONES of OS_ZONE words, zone = [OS_TICKETS ticket words | RADIX * OS_NSEG segment counts].
// Pass p reads its digit's counts from zone z and writes the next digit's counts -- and takes its tickets -- in zone z + 1.
// Every pass has a zone of its own and ONE memset in front of the sort zeroes them all (a memset per pass was a 5 us launch
// per pass: eight of them in the initial sort of a 1 MiB text, whose passes take 40 us).
// ------------------------------------------------------------------------------------------
// Tile shapes (threads, keys per thread, values through the keys' LDS buffer, workgroups per CU).  SA_AMD_ONESWEEP64_SHAPE /
// SA_AMD_ONESWEEP32_SHAPE select one for A/B measurements; every shape sorts correctly.
struct OsShape { int threads, items; bool seq; int wg_per_cu; };
static const OsShape os_shapes64[] = { { 1024, 8, false, 1 }, { 512, 16, true, 2 }, { 512, 8, false, 2 } };
static const OsShape os_shapes32[] = { { 1024, 12, false, 1 }, { 512, 16, true, 2 }, { 512, 12, false, 2 }, { 1024, 8, false, 1 } };
// (measured slower at 256 MiB, profiles/r03_onesweep_shapes.txt: 1024 x 16 and larger tiles -- spills at the 128-register limit of a
// 1024-thread workgroup --, 512 x 24 likewise; two workgroups per CU bought nothing at equal tile size)
constexpr int N_OS_SHAPES64 = (int)(sizeof(os_shapes64) / sizeof(os_shapes64[0]));
constexpr int N_OS_SHAPES32 = (int)(sizeof(os_shapes32) / sizeof(os_shapes32[0]));
constexpr int OS_TICKETS = 64;                 // words in front of a zone's counts: one ticket counter per segment
constexpr int OS_MAX_RADIX = 512;              // widest digit of the single-pass scatter (9 bits: the two passes in front of the bucket sort of large texts)
constexpr int OS_ZONE = OS_TICKETS + OS_MAX_RADIX * OS_NSEG;  // words
static_assert(OS_NSEG <= OS_TICKETS, "one ticket word per segment");
constexpr int OS_MAX_ZONES = 2 * 8 + 2;         // eight passes, each possibly behind a skipped one that needed a recount, + the producer's zone
static_assert(OS_MAX_ZONES * OS_ZONE <= RADIX * SORT_MAX_WG, "the zones live in the spine slab");

#ifdef SA_AMD_DIAG
static bool onesweep_on(const SortScratch &ss, const Tuning &tn) { return ss.status != nullptr && !tn.no_onesweep; }
#else
static bool onesweep_on(const SortScratch &ss, const Tuning &) { return ss.status != nullptr; }      // (the product's only engine)
#endif

struct OnesweepGeom { int tiles, nseg, tiles_per_seg; int64_t seg_elems; };
static OnesweepGeom onesweep_geom(int64_t count, int tile)
{
    OnesweepGeom g;
    g.tiles = (int)ceil_div(count, tile);
    if (g.tiles < 1) g.tiles = 1;
    int nseg = g.tiles < OS_NSEG ? g.tiles : OS_NSEG;
    g.tiles_per_seg = (int)ceil_div(g.tiles, nseg);
    g.nseg = (int)ceil_div(g.tiles, g.tiles_per_seg);
    g.seg_elems = (int64_t)g.tiles_per_seg * tile;
    return g;
}

// Where a producer of the keys adds the counts of the first pass's digit (k_build_keys: counts[d * G + chunk]), for the
// sort that will run on `count` pairs with this scratch: pointer, chunk size in elements, chunks.  The producer's stream
// must zero *zero_bytes bytes at *zero_ptr first.
struct FirstCounts { uint32_t *counts; int64_t chunk_elems; int G; void *zero_ptr; size_t zero_bytes; };
static FirstCounts sort_first_counts(const SortScratch &ss, const Tuning &tn, int64_t count, bool keys32);

static int cu_count()
{
    static int cus = 0;
    if (cus > 0) return cus;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    else { (void)hipGetLastError(); cus = 256; }
    return cus;
}

static int read_words(void *dst, const void *dsrc, size_t bytes, hipStream_t st);

__global__ __launch_bounds__(RADIX) void k_os_digit_totals(const uint32_t *__restrict__ hist, int nseg, uint32_t *__restrict__ digit_tot)
{
    uint32_t s = 0;
    for (int q = 0; q < nseg; ++q) s += hist[threadIdx.x * nseg + q];
    digit_tot[threadIdx.x] = s;
}

// Short sorts (fewer than SA_AMD_COUNT_NEXT_MIN_N pairs): ONE segment, and the counts of EVERY pass's digit from one read of the
// keys in front of the first pass -- a digit's totals do not depend on the order the pairs are in, and with one segment the
// totals are all a pass needs.  (Per pass either a counting kernel of its own, 7 us, or the flush of the in-pass count, more:
// 1 MiB of random bytes, five passes: 0.26 -> 0.23 ms.)
constexpr int HA_THREADS = 256;
template <typename KeyT>
__global__ __launch_bounds__(HA_THREADS) void k_radix_hist_all(const KeyT *__restrict__ keys, int64_t count, int begin_bit, int end_bit,
                                                               uint32_t *__restrict__ zone0, int zone_words, int ticket_words)
{
    __shared__ uint32_t h[8][RADIX];
    for (int i = threadIdx.x; i < 8 * RADIX; i += HA_THREADS) (&h[0][0])[i] = 0;
    __syncthreads();
    const int np = (end_bit - begin_bit + RADIX_BITS - 1) / RADIX_BITS;      // (<= 8, host-checked)
    for (int64_t i = (int64_t)blockIdx.x * HA_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * HA_THREADS) {
        const uint64_t k = (uint64_t)keys[i];
        for (int p = 0; p < np; ++p) {
            const int sh = begin_bit + p * RADIX_BITS, nb = end_bit - sh < RADIX_BITS ? end_bit - sh : RADIX_BITS;
            atomicAdd(&h[p][(k >> sh) & ((1u << nb) - 1u)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * RADIX; i += HA_THREADS) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&zone0[(size_t)(i / RADIX) * zone_words + ticket_words + (i % RADIX)], c);      // (one segment: counts[d * 1 + 0])
    }
}

template <typename KeyT, int THREADS, int ITEMS, bool SEQ, int RBITS = RADIX_BITS>
static int sort_pairs_onesweep(KeyT *keys_in, uint32_t *vals_in, KeyT *keys_alt, uint32_t *vals_alt, int64_t count, int begin_bit, int end_bit,
                               const SortScratch &ss, uint32_t *final_vals, hipStream_t st, KeyT **keys_res, uint32_t **vals_res, int *passes,
                               int *skipped, const Tuning &tn, bool iota, bool may_skip, bool first_counted,
                               const uint8_t *text = nullptr, int64_t text_n = 0,      // != nullptr (32-bit keys only): the FIRST pass reads its keys from the text (k_onesweep<..., TEXT_KEYS>)
                               int text_bits = 8,                                      //   8: the text itself (all 256 byte values), 2: the bit-packed text of a four-symbol alphabet
                               int val_extra = 0,                                      //   the first pass puts that many key bits below the 32 into the top bits of the values (OnesweepPass::val_extra)
                               KeyT *keys_out2 = nullptr,                              // != nullptr: keys_in is read-only -- the second pass writes its keys here, not into keys_in
                               uint8_t *head_flags = nullptr,                          // != nullptr (64-bit keys, final_vals): the last pass writes `count` group-start flags here and only the keys at
                                                                                       //   the ends of its tiles' digit runs (k_onesweep<..., HEAD_FLAGS>); the rest of *keys_res is then unspecified
                               bool poison_keys = false)                               // diagnostic library: fill that pass's key buffer with 0xA5 bytes first (sa_amd_test_sort_pairs_flags)
{
    constexpr int TILE = THREADS * ITEMS;
    constexpr int R = 1 << RBITS;
    static_assert(R <= OS_MAX_RADIX && (RBITS == RADIX_BITS || TILE >= 2 * OS_MIN_TILE), "zones and granule slab are sized for 8-bit digits of 4 Ki-element tiles");
    static_assert(TILE >= OS_MIN_TILE, "the granule slab is sized for tiles of at least OS_MIN_TILE elements");
    constexpr bool K64 = sizeof(KeyT) == 8;
    OnesweepGeom g = onesweep_geom(count, TILE);
    auto zone = [&](int i) { return ss.spine + (size_t)i * OS_ZONE; };
    int z = 0;                                    // zone that holds (or will hold) the counts of the coming pass's digit
    bool have_counts = first_counted;
    const int npass = (int)ceil_div(end_bit - begin_bit, RBITS);
    // every pass's counts up front (k_radix_hist_all): short sorts of keys that exist as an array, no pass to be skipped
    const bool upfront = RBITS == RADIX_BITS && !tn.no_upfront_counts && count < tn.count_next_min_n && !may_skip && !text && npass <= 8 && npass >= 2;
    if (upfront) { g.nseg = 1; g.tiles_per_seg = g.tiles; g.seg_elems = (int64_t)g.tiles * TILE; }
    HIP_TRY(hipMemsetAsync(ss.status, 0, (size_t)g.tiles * R * 8, st));
    {
        // zone 0 holds the producer's counts (first_counted) and stays; everything behind it starts from zero
        int zones = (may_skip ? 2 * npass : npass) + 1;
        if (zones > OS_MAX_ZONES) return SA_AMD_EINTERNAL;
        const int z0 = (first_counted && !upfront) ? 1 : 0;      // (up front: the producer counted per segment of another geometry -- counted again)
        HIP_TRY(hipMemsetAsync(zone(z0), 0, (size_t)(zones - z0) * OS_ZONE * 4, st));
    }
    if (upfront) {
        int blocks = (int)ceil_div(count, (int64_t)HA_THREADS * 16);
        if (blocks > 512) blocks = 512;
        if (blocks < 1) blocks = 1;
        PROF(K64 ? KC_UPSWEEP : KC_UPSWEEP32, count, st, hipLaunchKernelGGL((k_radix_hist_all<KeyT>), dim3((unsigned)blocks), dim3(HA_THREADS), 0, st, (const KeyT *)keys_in, count,
                                                                        begin_bit, end_bit, zone(0), (int)OS_ZONE, (int)OS_TICKETS));
        have_counts = true;
    }
    KeyT *kin = keys_in, *kout = keys_alt;
    uint32_t *vin = vals_in, *vout = vals_alt;
    constexpr int WG_PER_CU = THREADS <= 512 ? 2 : 1;
    int grid = cu_count() * WG_PER_CU;
    if (grid > g.tiles) grid = g.tiles;
    uint32_t epoch = 0;
    for (int shift = begin_bit; shift < end_bit; shift += RBITS) {
        const int nb = (end_bit - shift) < RBITS ? (end_bit - shift) : RBITS;
        const uint32_t dmask = (1u << nb) - 1u;
        const bool last = shift + RBITS >= end_bit;
        uint32_t *vdst = (last && final_vals) ? final_vals : vout;
        if (!have_counts) {
            if (RBITS != RADIX_BITS) return SA_AMD_EINTERNAL;     // (the counting kernels have 256 bins: a wide-digit sort gets its first counts from the producer of the keys)
            // one read of the keys for the counts of this digit (first pass of a sort whose producer did not count, or the
            // pass after a skipped one); zone z is still zero
            int split = 2048 / g.nseg;
            while (split > 1 && g.seg_elems / split < 8192) split /= 2;
            const int64_t sub = K64 ? ((ceil_div(g.seg_elems, split) + 1) & ~(int64_t)1) : ((ceil_div(g.seg_elems, split) + 3) & ~(int64_t)3);
            if (K64)
                PROF(KC_UPSWEEP, count, st, hipLaunchKernelGGL((k_radix_upsweep), dim3(g.nseg * split), dim3(SORT_THREADS), 0, st, (const uint64_t *)kin,
                                                               zone(z) + OS_TICKETS, count, shift, dmask, g.seg_elems, g.nseg, split, sub));
            else
                PROF(KC_UPSWEEP32, count, st, hipLaunchKernelGGL((k_radix_upsweep32), dim3(g.nseg * split), dim3(SORT_THREADS), 0, st, (const uint32_t *)kin,
                                                                 zone(z) + OS_TICKETS, count, shift, dmask, g.seg_elems, g.nseg, split, sub));
        }
        if (RBITS == RADIX_BITS && may_skip && !tn.no_run_skip && count >= tn.run_skip_min && !(iota && *passes == 0) && !(last && final_vals)) {
            // a digit that is the same for EVERY element makes the pass the identity (the sort is stable): skip it
            hipLaunchKernelGGL(k_os_digit_totals, dim3(1), dim3(RADIX), 0, st, (const uint32_t *)(zone(z) + OS_TICKETS), g.nseg, ss.digit_tot);
            LAUNCH_CHECK(st);
            uint32_t tot[RADIX];
            { const int rcw = read_words(tot, ss.digit_tot, sizeof(tot), st); if (rcw) return rcw; }
            bool constant = false;
            for (int d = 0; d < RADIX; ++d) constant |= (int64_t)tot[d] == count;
            if (constant) { ++*skipped; have_counts = false; ++z; continue; }     // (zone z holds the skipped digit's counts: the recount takes the next, clean one)
        }
        OnesweepPass P;
        P.hist_cur = zone(z) + OS_TICKETS;
        // (short inputs: the flush of the next digit's counts -- 256 x segments atomics per workgroup on the same few lines -- costs
        // more than a counting kernel of its own)
        // (measured, tools/midsize_knobs.py: 1 MiB of random bytes 0.420 -> 0.369 ms, 2 MiB of English 0.902 -> 0.777; the other way
        // round below 400 K pairs -- a launch more per pass -- and from 8 M on)
        const bool count_next = !upfront && !last && (RBITS != RADIX_BITS || count >= tn.count_next_min_n || count < tn.count_next_below_n);
        P.hist_next = count_next ? zone(z + 1) + OS_TICKETS : nullptr;
        P.tickets = zone(z + 1);
        P.status = ss.status;
        P.err = ss.err;
        P.n = count;
        P.shift = shift; P.dmask = dmask;
        P.shift_next = shift + RBITS;
        { const int nbn = (end_bit - P.shift_next) < RBITS ? (end_bit - P.shift_next) : RBITS; P.dmask_next = last ? 0u : (1u << nbn) - 1u; }
        P.nseg = g.nseg; P.tiles_per_seg = g.tiles_per_seg; P.tiles = g.tiles;
        P.epoch = ++epoch;
        P.flags = (uint32_t)tn.onesweep_flags;
        P.text = text; P.text_n = text_n; P.text_bits = text_bits;
        P.val_extra = (text && *passes == 0 && iota) ? val_extra : 0;
        // (the flags pass exists for 64-bit keys only: a 32-bit sort ignores head_flags, and so does every pass but the last)
        constexpr bool FLAGS_OK = K64 && RBITS == RADIX_BITS;
        P.head_flags = (FLAGS_OK && last && final_vals) ? head_flags : nullptr;
        if (P.head_flags) {
            if constexpr (FLAGS_OK) {
#ifdef SA_AMD_DIAG
                if (poison_keys) HIP_TRY(hipMemsetAsync(kout, 0xA5, (size_t)count * sizeof(KeyT), st));
#endif
                PROF(KC_ONESWEEP, count, st,
                     hipLaunchKernelGGL((k_onesweep<THREADS, ITEMS, KeyT, SEQ, WG_PER_CU, RBITS, false, true>), dim3(grid), dim3(THREADS), 0, st, (const KeyT *)kin,
                                        (const uint32_t *)((iota && *passes == 0) ? nullptr : vin), kout, vdst, P));
            }
        } else if (!K64 && !SEQ && text && *passes == 0)
            PROF(KC_ONESWEEP32, count, st,
                 hipLaunchKernelGGL((k_onesweep<THREADS, ITEMS, KeyT, SEQ, WG_PER_CU, RBITS, !K64 && !SEQ>), dim3(grid), dim3(THREADS), 0, st, (const KeyT *)kin,
                                    (const uint32_t *)((iota && *passes == 0) ? nullptr : vin), kout, vdst, P));
        else
        PROF(K64 ? KC_ONESWEEP : KC_ONESWEEP32, count, st,
             hipLaunchKernelGGL((k_onesweep<THREADS, ITEMS, KeyT, SEQ, WG_PER_CU, RBITS>), dim3(grid), dim3(THREADS), 0, st, (const KeyT *)kin,
                                (const uint32_t *)((iota && *passes == 0) ? nullptr : vin), kout, vdst, P));
        KeyT *tk = kin; kin = kout; kout = (keys_out2 && *passes == 0) ? keys_out2 : tk;
        uint32_t *free_v = vin;                   // the values just consumed become the next scratch target
        vin = vdst;
        vout = free_v;
        ++*passes;
        ++z;
        have_counts = count_next || upfront;
    }
    *keys_res = kin; *vals_res = vin;
    return SA_AMD_OK;
}

struct SortResult { uint64_t *keys; uint32_t *vals; int passes; int skipped; };

// stable LSD sort of `count` pairs on key bits [begin_bit, end_bit); ping-pongs between in/alt.
// spine: RADIX * SORT_MAX_WG words, digit_tot: RADIX words.  final_vals (optional): the LAST pass
// writes its values there instead of into the ping-pong buffer (the initial sort delivers
// straight into SA this way).
static int sort_pairs(uint64_t *keys_in, uint32_t *vals_in, uint64_t *keys_alt, uint32_t *vals_alt, int64_t count,
                      int begin_bit, int end_bit, const SortScratch &ss, uint32_t *final_vals,
                      hipStream_t st, SortResult *res, const Tuning &tn, bool iota = false,   // iota: value i = index i, vals_in is scratch only
                      bool may_skip = false,                                                   // look for passes that are the identity (costs a read-back per pass)
                      bool first_counted = false,                                              // the producer of keys_in has histogrammed the first digit (sort_first_counts says where and how)
                      uint8_t *head_flags = nullptr, bool poison_keys = false)                 // single-pass engine only, with final_vals: see sort_pairs_onesweep
{
    res->keys = keys_in; res->vals = vals_in; res->passes = 0; res->skipped = 0;
    if (count <= 1 || end_bit <= begin_bit) return SA_AMD_OK;
    if (onesweep_on(ss, tn)) {
#define OS_CALL64(T, I, S) sort_pairs_onesweep<uint64_t, T, I, S>(keys_in, vals_in, keys_alt, vals_alt, count, begin_bit, end_bit, ss, final_vals, st, \
                                                                 &res->keys, &res->vals, &res->passes, &res->skipped, tn, iota, may_skip, first_counted, \
                                                                 nullptr, 0, 8, 0, nullptr, head_flags, poison_keys)
        switch (tn.onesweep64_shape) {
        case 1: return OS_CALL64(512, 16, true);
        case 2: return OS_CALL64(512, 8, false);
        default: return OS_CALL64(1024, 8, false);
        }
#undef OS_CALL64
    }
#ifdef SA_AMD_DIAG
    uint32_t *spine = ss.spine, *digit_tot = ss.digit_tot;
    const SortVariant &sv = sort_variants[tn.sort_variant];
    const SortGrid g = sort_grid(count, sv);
    uint64_t *kin = keys_in, *kout = keys_alt;
    uint32_t *vin = vals_in, *vout = vals_alt;
    for (int shift = begin_bit; shift < end_bit; shift += RADIX_BITS) {
        const int nb = (end_bit - shift) < RADIX_BITS ? (end_bit - shift) : RADIX_BITS;
        const uint32_t dmask = (1u << nb) - 1u;
        const bool last = shift + RADIX_BITS >= end_bit;
        uint32_t *vdst = (last && final_vals) ? final_vals : vout;
        {
            const int64_t chunk = g.tiles_per_wg * g.tile;
            int split = 2048 / g.G;
            if (split < 1) split = 1;
            while (split > 1 && chunk / split < 4096) split /= 2;
            const int64_t sub = (ceil_div(chunk, split) + 1) & ~(int64_t)1;
            // (atomic accumulation needs a zeroed spine: once here, afterwards every downsweep zeroes what it consumed)
            if (first_counted && shift == begin_bit) {
                // (nothing to do: k_build_keys has added this pass's digit counts to the spine)
            } else {
            if (split > 1 && res->passes == 0) HIP_TRY(hipMemsetAsync(spine, 0, (size_t)RADIX * g.G * 4, st));
            PROF(KC_UPSWEEP, count, st, hipLaunchKernelGGL((k_radix_upsweep), dim3(g.G * split), dim3(SORT_THREADS), 0, st, kin, spine,
                                                           count, shift, dmask, chunk, g.G, split, sub));
            }
        }
        PROF(KC_SPINE, (int64_t)RADIX * g.G, st, hipLaunchKernelGGL((k_spine_rows), dim3(RADIX), dim3(SPINE_THREADS), 0, st,
                                                                    spine, digit_tot, g.G));
        // A digit that is the same for EVERY element makes the pass the identity (the sort is stable): skip the tile scatter.
        // Worth a 1 KiB read-back (a host round trip of ~30 us) only for the large global sorts of the refinement rounds: texts
        // that are one run or one period keep hundreds of millions of suffixes in a few groups round after round, and their
        // (group, rank) keys are constant in most digits.  The ISA passes never look, the initial sort only for a text of one byte value.
        if (may_skip && !tn.no_run_skip && count >= tn.run_skip_min && !(iota && res->passes == 0) && !(last && final_vals)) {
            uint32_t tot[RADIX];
            { const int rcw = read_words(tot, digit_tot, sizeof(tot), st); if (rcw) return rcw; }
            bool constant = false;
            for (int d = 0; d < RADIX; ++d) constant |= (int64_t)tot[d] == count;
            if (constant) {
                HIP_TRY(hipMemsetAsync(spine, 0, (size_t)RADIX * g.G * 4, st));     // (the tile scatter would have zeroed what it consumed)
                res->skipped++;
                continue;
            }
        }
        PROF(KC_DOWNSWEEP, count, st, hipLaunchKernelGGL((sv.fn), dim3(g.G), dim3(sv.threads), 0, st,
                                                         (const uint64_t *)kin, (const uint32_t *)((iota && res->passes == 0) ? nullptr : vin), kout, vdst,
                                                         spine, (const uint32_t *)digit_tot, count, shift,
                                                         dmask, g.tiles_per_wg, g.G));
        uint64_t *tk = kin; kin = kout; kout = tk;
        uint32_t *free_v = vin;     // the values just consumed become the next scratch target
        vin = vdst;
        vout = free_v;
        res->passes++;
    }
    res->keys = kin; res->vals = vin;
    return SA_AMD_OK;
#else
    return SA_AMD_EINTERNAL;        // (no scratch for the single-pass scatter: cannot happen, every caller carves it)
#endif
}

struct SortResult32 { uint32_t *keys; uint32_t *vals; int passes; };
#ifdef SA_AMD_DIAG
// 32-bit keys (two-stage initial sort): same three-kernel pass, 12 Ki-pair tiles by default (the LDS stage holds more 4-byte elements)
constexpr int SORT32_THREADS = 1024;
typedef void (*Downsweep32Fn)(const uint32_t *, const uint32_t *, uint32_t *, uint32_t *, uint32_t *, const uint32_t *, int64_t, int,
                              uint32_t, int64_t, int);
struct Sort32Variant { int items; Downsweep32Fn fn; };
static const Sort32Variant sort32_variants[] = {
    { 12, k_radix_downsweep_wcl<SORT32_THREADS, 12, 16, 1, false, uint32_t, 12> },    // default: next tile's keys prefetched into LDS
    { 12, k_radix_downsweep_wcl<SORT32_THREADS, 12, 16, 1, false, uint32_t> },
    { 8, k_radix_downsweep_wcl<SORT32_THREADS, 8, 16, 1, false, uint32_t> },
    { 16, k_radix_downsweep_wcl<SORT32_THREADS, 16, 16, 1, false, uint32_t> },        // spills
    { 8, k_radix_downsweep_wcl<SORT32_THREADS, 8, 16, 1, false, uint32_t, 8> },
    // (two workgroups per CU: 1024 x 4 or 1024 x 8 with granule 8 and 64 VGPRs measured slower, 8.6 -> 9.0 .. 10.2 ms at 256 MiB)
};
constexpr int N_SORT32_VARIANTS = (int)(sizeof(sort32_variants) / sizeof(sort32_variants[0]));

struct SortGrid32 { int G; int64_t tiles_per_wg, tile; };
static SortGrid32 sort_grid32(int64_t count, const Sort32Variant &sv)
{
    SortGrid32 g;
    g.tile = (int64_t)SORT32_THREADS * sv.items;
    const int64_t tiles = ceil_div(count, g.tile);
    g.tiles_per_wg = ceil_div(tiles, 512);
    if (g.tiles_per_wg < 1) g.tiles_per_wg = 1;
    g.G = (int)ceil_div(tiles, g.tiles_per_wg);
    return g;
}

#else
constexpr int N_SORT32_VARIANTS = 1;
#endif

static int sort_pairs32(uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_alt, uint32_t *vals_alt, int64_t count, int begin_bit,
                        int end_bit, const SortScratch &ss, uint32_t *final_vals, hipStream_t st, SortResult32 *res,
                        const Tuning &tn, bool iota = false, bool first_counted = false,
                        int rbits = RADIX_BITS,       // 9: nine-bit digits (single-pass engine only, first digit counted by the producer)
                        const uint8_t *text = nullptr, int64_t text_n = 0, int text_bits = 8,      // the first pass reads its keys from this text (single-pass engine, default tile, counted)
                        int val_extra = 0,
                        uint32_t *keys_out2 = nullptr)      // != nullptr: keys_in is read-only, the second pass writes its keys here (sort_pairs_onesweep)
{
    res->keys = keys_in; res->vals = vals_in; res->passes = 0;
    if (keys_out2 && (rbits != RADIX_BITS || text)) return SA_AMD_EINTERNAL;
    if (count <= 1 || end_bit <= begin_bit) return SA_AMD_OK;
    if (rbits != RADIX_BITS && (rbits != 9 || !onesweep_on(ss, tn) || !first_counted)) return SA_AMD_EINTERNAL;
    if (text && (!onesweep_on(ss, tn) || !first_counted || tn.onesweep32_shape != 0)) return SA_AMD_EINTERNAL;
    if (onesweep_on(ss, tn)) {
        int skipped = 0;
        if (rbits == 9)
            return sort_pairs_onesweep<uint32_t, 1024, 12, false, 9>(keys_in, vals_in, keys_alt, vals_alt, count, begin_bit, end_bit, ss, final_vals, st,
                                                                     &res->keys, &res->vals, &res->passes, &skipped, tn, iota, false, first_counted, text, text_n, text_bits, val_extra);
        if (text)
            return sort_pairs_onesweep<uint32_t, 1024, 12, false, RADIX_BITS>(keys_in, vals_in, keys_alt, vals_alt, count, begin_bit, end_bit, ss, final_vals, st,
                                                                              &res->keys, &res->vals, &res->passes, &skipped, tn, iota, false, first_counted, text, text_n, text_bits, val_extra);
#define OS_CALL32(T, I, S) sort_pairs_onesweep<uint32_t, T, I, S>(keys_in, vals_in, keys_alt, vals_alt, count, begin_bit, end_bit, ss, final_vals, st, \
                                                                 &res->keys, &res->vals, &res->passes, &skipped, tn, iota, false, first_counted, \
                                                                 nullptr, 0, 8, 0, keys_out2)
        switch (tn.onesweep32_shape) {
        case 1: return OS_CALL32(512, 16, true);
        case 2: return OS_CALL32(512, 12, false);
        case 3: return OS_CALL32(1024, 8, false);
        default: return OS_CALL32(1024, 12, false);
        }
#undef OS_CALL32
    }
#ifdef SA_AMD_DIAG
    uint32_t *spine = ss.spine, *digit_tot = ss.digit_tot;
    const Sort32Variant &sv = sort32_variants[tn.sort32_variant];
    const SortGrid32 g32 = sort_grid32(count, sv);
    const int64_t SORT32_TILE = g32.tile, tiles_per_wg = g32.tiles_per_wg;
    const int G = g32.G;
    uint32_t *kin = keys_in, *kout = keys_alt, *vin = vals_in, *vout = vals_alt;
    for (int shift = begin_bit; shift < end_bit; shift += RADIX_BITS) {
        const int nb = (end_bit - shift) < RADIX_BITS ? (end_bit - shift) : RADIX_BITS;
        const uint32_t dmask = (1u << nb) - 1u;
        const bool last = shift + RADIX_BITS >= end_bit;
        uint32_t *vdst = (last && final_vals) ? final_vals : vout;
        {
            const int64_t chunk = tiles_per_wg * SORT32_TILE;
            int split = 2048 / G;
            if (split < 1) split = 1;
            while (split > 1 && chunk / split < 8192) split /= 2;
            const int64_t sub = (ceil_div(chunk, split) + 3) & ~(int64_t)3;
            if (first_counted && shift == begin_bit) {
                // (k_build_keys has added this pass's digit counts to the spine)
            } else {
            if (split > 1 && res->passes == 0) HIP_TRY(hipMemsetAsync(spine, 0, (size_t)RADIX * G * 4, st));
            PROF(KC_UPSWEEP32, count, st, hipLaunchKernelGGL((k_radix_upsweep32), dim3(G * split), dim3(SORT_THREADS), 0, st,
                                                           (const uint32_t *)kin, spine, count, shift, dmask, chunk, G, split, sub));
            }
        }
        PROF(KC_SPINE, (int64_t)RADIX * G, st, hipLaunchKernelGGL((k_spine_rows), dim3(RADIX), dim3(SPINE_THREADS), 0, st, spine, digit_tot, G));
        PROF(KC_DOWNSWEEP32, count, st, hipLaunchKernelGGL((sv.fn),
                                                         dim3(G), dim3(SORT32_THREADS), 0, st, (const uint32_t *)kin,
                                                         (const uint32_t *)((iota && res->passes == 0) ? nullptr : vin), kout,
                                                         vdst, spine, (const uint32_t *)digit_tot, count, shift, dmask,
                                                         tiles_per_wg, G));
        uint32_t *tk = kin; kin = kout; kout = (keys_out2 && res->passes == 0) ? keys_out2 : tk;
        uint32_t *free_v = vin;
        vin = vdst;
        vout = free_v;
        res->passes++;
    }
    res->keys = kin; res->vals = vin;
    return SA_AMD_OK;
#else
    return SA_AMD_EINTERNAL;
#endif
}

static FirstCounts sort_first_counts(const SortScratch &ss, const Tuning &tn, int64_t count, bool keys32)
{
    FirstCounts f;
    if (onesweep_on(ss, tn)) {
        const OsShape &sh = keys32 ? os_shapes32[tn.onesweep32_shape] : os_shapes64[tn.onesweep64_shape];
        const int tile = sh.threads * sh.items;
        const OnesweepGeom g = onesweep_geom(count, tile);
        f.counts = ss.spine + OS_TICKETS; f.chunk_elems = g.seg_elems; f.G = g.nseg;
        f.zero_ptr = ss.spine; f.zero_bytes = (size_t)OS_ZONE * 4;
        return f;
    }
#ifdef SA_AMD_DIAG
    f.counts = ss.spine; f.zero_ptr = ss.spine;
    if (keys32) {
        const SortGrid32 g32 = sort_grid32(count, sort32_variants[tn.sort32_variant]);
        f.chunk_elems = g32.tiles_per_wg * g32.tile; f.G = g32.G;
    } else {
        const SortGrid g64 = sort_grid(count, sort_variants[tn.sort_variant]);
        f.chunk_elems = g64.tiles_per_wg * g64.tile; f.G = g64.G;
    }
    f.zero_bytes = (size_t)RADIX * f.G * 4;
    return f;
#else
    f.counts = ss.spine; f.zero_ptr = ss.spine; f.chunk_elems = count; f.G = 1; f.zero_bytes = (size_t)RADIX * 4;      // (not reached)
    return f;
#endif
}

// ------------------------------------------------------------------------------------------
// Bucket sort of the 32-bit first stage (kernels/bucket_sort.hpp): pairs grouped by their top 16 key bits (two stable
// global passes) -> pairs in the order of the whole 32-bit key, one workgroup per bucket, everything in LDS.
// ------------------------------------------------------------------------------------------
struct BkShape { int threads, items, minw; };
// (threads, pairs per thread, waves per SIMD the registers are held to); the first three are the ones in use -- the smallest that
// holds the largest bucket is taken --, the last is kept for A/B measurements (SA_AMD_BUCKET_SHAPE tries that one first)
static const BkShape bk_shapes[] = { { 256, 10, 6 }, { 512, 10, 8 }, { 1024, 10, 8 }, { 1024, 20, 1 }, { 256, 20, 1 } };
constexpr int N_BK_SHAPES = (int)(sizeof(bk_shapes) / sizeof(bk_shapes[0]));
constexpr int N_BK_DEFAULT = 4;
static int64_t bucket_cap(int shape) { return (int64_t)bk_shapes[shape].threads * bk_shapes[shape].items; }
static int64_t bucket_cap_max() { return bucket_cap(N_BK_DEFAULT - 1); }

// top_bits: 16 or 18 key bits that the global passes have ordered.  *done = false: some bucket is larger than every shape holds
// (nothing was written; the caller sorts the low bits globally).  words: two scratch words (largest bucket, error count);
// start: 2^top_bits + 1 words.  Read-back: the largest bucket.
// fin != nullptr: the tied suffixes are ordered by their low key bits in the same launch (what k_finish_sorted does in a pass of
// its own) when the shape has room to do it well (*fused); the caller has zeroed fin's bitmap and counters.
static int bucket_sort32(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out, int64_t count, int top_bits,
                         uint32_t *start, uint32_t *words, hipStream_t st, const Tuning &tn, bool *done, uint32_t *largest,
                         const BucketFinish *fin = nullptr, const KeyParams *P = nullptr, const KeySrc *K = nullptr, bool *fused = nullptr,
                         int val_extra = 0)      // the top val_extra bits of every value are the key bits below the 32 (ordered with them, stripped on the way out)
{
    *done = false; *largest = 0;
    if (fused) *fused = false;
    if (top_bits < 32 - BK_MAX_LBITS || top_bits > BK_TOP_BITS_MAX) return SA_AMD_EINTERNAL;
    const int lbits = 32 - top_bits;
    if (val_extra < 0 || lbits + val_extra > BK_MAX_LBITS) return SA_AMD_EINTERNAL;
    const uint32_t nb = 1u << top_bits;
    HIP_TRY(hipMemsetAsync(words, 0, 8, st));
    PROF(KC_MISC, nb, st, hipLaunchKernelGGL((k_bucket_starts), dim3((unsigned)ceil_div((int64_t)nb + 1, BK_STARTS_THREADS)), dim3(BK_STARTS_THREADS),
                                              0, st, keys_in, count, lbits, nb, start));
    PROF(KC_MISC, nb, st, hipLaunchKernelGGL((k_bucket_max), dim3((unsigned)ceil_div((int64_t)nb, BK_STARTS_THREADS)), dim3(BK_STARTS_THREADS), 0, st,
                                              (const uint32_t *)start, nb, words));
    uint32_t maxb = 0;
    { const int rcw = read_words(&maxb, words, 4, st); if (rcw) return rcw; }
    *largest = maxb;
    int shape = -1;
    if (tn.bucket_shape >= 0 && tn.bucket_shape < N_BK_SHAPES && bucket_cap(tn.bucket_shape) >= (int64_t)maxb) shape = tn.bucket_shape;
    for (int c = 0; shape < 0 && c < N_BK_DEFAULT; ++c)
        if (bucket_cap(c) >= (int64_t)maxb) shape = c;
    if (shape < 0) return SA_AMD_OK;
    // the 20-pairs-per-thread shapes leave one workgroup per CU (or three waves per SIMD): the tied suffixes' text look-ups have
    // nothing to hide behind there (1 GiB DNA: 7.7 + 7.5 ms as two kernels, 16.9 ms fused) -- k_finish_sorted follows instead
    const bool fuse = fin != nullptr && (bk_shapes[shape].items <= 10 || tn.bucket_finish_always);
    const BucketFinish F0 = BucketFinish();
    const KeyParams P0 = KeyParams();
    const KeySrc K0 = KeySrc();
#define BK_LAUNCH(T, I, W)                                                                                                               \
    do {                                                                                                                                 \
        if (fuse) PROF(KC_BUCKET, count, st, hipLaunchKernelGGL((k_bucket_sort<T, I, W, true>), dim3(nb), dim3(T), 0, st, keys_in, vals_in,         \
                                                                (const uint32_t *)start, lbits, keys_out, vals_out, words + 1, *fin, *P, *K, val_extra)); \
        else PROF(KC_BUCKET, count, st, hipLaunchKernelGGL((k_bucket_sort<T, I, W, false>), dim3(nb), dim3(T), 0, st, keys_in, vals_in,             \
                                                            (const uint32_t *)start, lbits, keys_out, vals_out, words + 1, F0, P0, K0, val_extra)); \
    } while (0)
    switch (shape) {
    case 0: BK_LAUNCH(256, 10, 6); break;
    case 1: BK_LAUNCH(512, 10, 8); break;
    case 2: BK_LAUNCH(1024, 10, 8); break;
    case 3: BK_LAUNCH(1024, 20, 1); break;
    default: BK_LAUNCH(256, 20, 1); break;
    }
#undef BK_LAUNCH
    *done = true;
    if (fused) *fused = fuse;
    return SA_AMD_OK;
}

#ifdef SA_AMD_DIAG
// ------------------------------------------------------------------------------------------
// Sample sort of the 64-bit stage (kernels/sample_sort.hpp): (key, i) pairs of keys_a[0 .. n) -> keys in order in keys_b, the
// suffixes in final_vals.  Scratch: keys_c (the sample and its sort), vals_a / vals_b (the values between the levels), u0 / u1
// (values of the sample's sort), big (n / 8 + 1 MiB bytes at least: the tiles' counts), small (2 MiB: totals, bases, segments,
// tile descriptors come behind), words (two counters + the list of reported buckets).
// *done = false: some bucket that is no equality bucket did not fit a workgroup (keys_a no longer holds the keys): the caller
// builds the keys again and sorts them with the LSD engine.  One read-back (the reported buckets).
// ------------------------------------------------------------------------------------------
static int64_t sample_count(int64_t n, const Tuning &tn)
{
    int lg = tn.sample_log ? tn.sample_log : (n >= ((int64_t)1 << 28) ? 22 : (n >= ((int64_t)1 << 27) ? 21 : 20));
    while (lg > 16 && ((int64_t)1 << lg) * 4 > n) --lg;
    return (int64_t)1 << lg;
}

static int sample_sort64(uint64_t *keys_a, uint64_t *keys_b, uint64_t *keys_c, uint32_t *vals_a, uint32_t *vals_b, uint32_t *u0, uint32_t *u1,
                         uint32_t *big, uint32_t *small, uint32_t *words, uint32_t *final_vals, int64_t n, int key_bits, const SortScratch &ss,
                         hipStream_t st, sa_amd_stats *local, const Tuning &tn, bool *done, bool trace)
{
    *done = false;
    const int64_t S = sample_count(n, tn);
    if (S < 65536 || n < 4 * S || n >= ((int64_t)1 << 32)) return SA_AMD_OK;
    // ---- the sample, sorted (its values are scratch) ----
    uint64_t *samp = keys_c, *samp_alt = keys_c + S;
    PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_ss_sample), dim3((unsigned)ceil_div(S, 256)), dim3(256), 0, st, (const uint64_t *)keys_a, n, S, samp));
    SortResult sr;
    int rc = sort_pairs(samp, u0, samp_alt, u1, S, 0, key_bits, ss, nullptr, st, &sr, tn, true);
    if (rc) return rc;
    local->sort_passes += sr.passes; local->sorted_elements += (int64_t)sr.passes * S;
    const uint64_t *sample = sr.keys;
    // ---- scratch layout ----
    const int64_t tiles1 = ceil_div(n, SS_TILE), max_tiles2 = tiles1 + SS_WAYS;
    const int64_t per = ceil_div(tiles1, SS_CHUNKS);
    const int chunks = (int)ceil_div(tiles1, per);
    uint32_t *counts = big;                                            // level 1: tiles1 x 256, level 2: max_tiles2 x 512
    uint32_t *tot1 = small, *base1 = tot1 + SS_CHUNKS * SS_WAYS, *seg_start = base1 + SS_CHUNKS * SS_WAYS, *seg_first = seg_start + 320;
    uint32_t *tot2 = seg_first + 320, *bstart = tot2 + SS_WAYS * SS_IDS2;
    uint32_t *tile_seg = bstart + SS_BUCKETS + 64, *tile_base = tile_seg + ((max_tiles2 + 63) & ~(int64_t)63);
    // ---- level 1 ----
    PROF(KC_SS_COUNT, n, st, hipLaunchKernelGGL((k_ss_count<1>), dim3((unsigned)tiles1), dim3(SS_THREADS), 0, st, (const uint64_t *)keys_a, n, sample, S,
                                                (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, counts));
    PROF(KC_RR_SCAN, tiles1, st, hipLaunchKernelGGL((k_ss_scan_tiles<SS_WAYS>), dim3((unsigned)chunks), dim3(SS_WAYS), 0, st, counts, tiles1, per,
                                                    (const uint32_t *)nullptr, tot1));
    PROF(KC_RR_SCAN, chunks, st, hipLaunchKernelGGL((k_ss_bases1), dim3(1), dim3(SS_WAYS), 0, st, (const uint32_t *)tot1, chunks, base1, seg_start, seg_first));
    PROF(KC_RR_SCAN, max_tiles2, st, hipLaunchKernelGGL((k_ss_tiles), dim3(SS_WAYS + 1), dim3(256), 0, st, (const uint32_t *)seg_start, (const uint32_t *)seg_first,
                                                        max_tiles2, tile_seg, tile_base));
    PROF(KC_SS_SCATTER, n, st, hipLaunchKernelGGL((k_ss_scatter<1>), dim3((unsigned)tiles1), dim3(SS_THREADS), 0, st, (const uint64_t *)keys_a, (const uint32_t *)nullptr, n,
                                                  sample, S, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                                                  (const uint32_t *)counts, (const uint32_t *)base1, per, keys_b, vals_a));
    // ---- level 2 (the pairs of a segment stay inside it: keys_b -> keys_a) ----
    PROF(KC_SS_COUNT, n, st, hipLaunchKernelGGL((k_ss_count<2>), dim3((unsigned)max_tiles2), dim3(SS_THREADS), 0, st, (const uint64_t *)keys_b, n, sample, S,
                                                (const uint32_t *)tile_seg, (const uint32_t *)tile_base, (const uint32_t *)seg_start, counts));
    PROF(KC_RR_SCAN, max_tiles2, st, hipLaunchKernelGGL((k_ss_scan_tiles<SS_IDS2>), dim3(SS_WAYS), dim3(SS_IDS2), 0, st, counts, max_tiles2, (int64_t)0,
                                                        (const uint32_t *)seg_first, tot2));
    PROF(KC_RR_SCAN, SS_WAYS, st, hipLaunchKernelGGL((k_ss_bases2), dim3(SS_WAYS), dim3(SS_IDS2), 0, st, (const uint32_t *)tot2, (const uint32_t *)seg_start, bstart, (uint32_t)n));
    PROF(KC_SS_SCATTER, n, st, hipLaunchKernelGGL((k_ss_scatter<2>), dim3((unsigned)max_tiles2), dim3(SS_THREADS), 0, st, (const uint64_t *)keys_b, (const uint32_t *)vals_a, n,
                                                  sample, S, (const uint32_t *)tile_seg, (const uint32_t *)tile_base, (const uint32_t *)seg_start,
                                                  (const uint32_t *)counts, (const uint32_t *)bstart, (int64_t)1, keys_a, vals_b));
    // ---- level 3: every bucket in LDS (keys_a -> keys_b, values -> final_vals) ----
    HIP_TRY(hipMemsetAsync(words, 0, 16, st));
    if (!tn.sample_merge)
    PROF(KC_SS_BUCKET, n, st, hipLaunchKernelGGL((k_ss_bucket_sort<SB_SMALL_THREADS, SB_SMALL_ITEMS, 9, 0, false>), dim3((unsigned)SS_BUCKETS), dim3(SB_SMALL_THREADS), 0, st,
                                                 (const uint64_t *)keys_a, (const uint32_t *)vals_b, (const uint32_t *)bstart, keys_b, final_vals, words, words + 4));
    else
    PROF(KC_SS_BUCKET, n, st, hipLaunchKernelGGL((k_ss_bucket_merge<SB_SMALL_THREADS, SB_SMALL_ITEMS>), dim3((unsigned)SS_BUCKETS), dim3(SB_SMALL_THREADS), 0, st,
                                                 (const uint64_t *)keys_a, (const uint32_t *)vals_b, (const uint32_t *)bstart, keys_b, final_vals, words));
    PROF(KC_SS_BUCKET, 0, st, hipLaunchKernelGGL((k_ss_bucket_sort<SB_THREADS, SB_ITEMS, 10, SB_SMALL_CAP, true>), dim3((unsigned)SS_BUCKETS), dim3(SB_THREADS), 0, st,
                                                 (const uint64_t *)keys_a, (const uint32_t *)vals_b, (const uint32_t *)bstart, keys_b, final_vals, words, words + 4));
    uint32_t res[2] = { 0, 0 };
    { const int rcw = read_words(res, words, 8, st); if (rcw) return rcw; }
    local->sort_passes += 3; local->sorted_elements += 3 * n;
    if (trace) fprintf(stderr, "suffix_array_amd: sample sort: %lld samples, largest bucket %u (a workgroup holds %d), %u oversize buckets that are no equality buckets\n",
                       (long long)S, res[1], SB_CAP, res[0]);
    *done = res[0] == 0;
    return SA_AMD_OK;
}

#endif  // SA_AMD_DIAG

}  // namespace sa
