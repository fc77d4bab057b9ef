// host/sort.hpp -- the radix-sort drivers of the device pipeline (host/pipeline.hpp, host/refine_round.hpp), the product's: what a sort needs (SortScratch),
// what it is asked (SortJob) and answers (SortResult), the single-pass tile scatter's host side (sort_pairs, sort_pairs32,
// sort_first_counts) and the in-LDS bucket sort of the 32-bit first stage (bucket_sort32).  The diagnostic library's second engine
// and its sample sort are in host/sort_diag.hpp.
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

// what a radix sort needs besides its ping-pong buffers
struct SortScratch {
    uint32_t *spine;                // RADIX * SORT_MAX_WG words: per-chunk counts (three-kernel pass) / two zones of segment counts + tickets (single-pass)
    uint32_t *digit_tot;            // RADIX words
    unsigned long long *status;     // single-pass scatter: 256 granules per tile (nullptr: the three-kernel pass is used)
    uint32_t *err;                  // single-pass scatter: look-back give-ups (must stay 0).  A tile whose look-back gave up (2^22 polls without
                                    // an answer: never seen, the bound turns a hang into an error) has scattered with a partial prefix -- in bounds,
                                    // wrong order --, so EVERY user of a SortScratch reads err[0] before it trusts a result: build_device at its end
                                    // (SA_AMD_EINTERNAL), sa_amd_check_integrity_device behind its sorts, the diagnostic hooks behind theirs
    // the two slabs a SortScratch is made of: spine + digit totals, and the granules of sorts of up to `count` pairs
    static constexpr size_t SPINE_BYTES = ((size_t)RADIX * SORT_MAX_WG + RADIX) * 4;
    static size_t granule_bytes(int64_t count) { return ((size_t)ceil_div(count, OS_MIN_TILE) + 1) * RADIX * 8; }
    // err: four words that the owner zeroes in front of its sorts (err[0]: the give-ups)
    static SortScratch make(void *spine_slab, void *granule_slab, uint32_t *err)
    {
        SortScratch ss;
        ss.spine = (uint32_t *)spine_slab;
        ss.digit_tot = ss.spine + (size_t)RADIX * SORT_MAX_WG;
        ss.status = (unsigned long long *)granule_slab;
        ss.err = err;
        return ss;
    }
};

// One stable LSD sort of `count` pairs on key bits [begin_bit, end_bit); ping-pongs between in/alt.  The first seven fields are
// every job's, a caller names the others only where it departs from the default.
template <typename KeyT>
struct SortJob {
    KeyT *keys_in; uint32_t *vals_in; KeyT *keys_alt; uint32_t *vals_alt;
    int64_t count;
    int begin_bit, end_bit;
    uint32_t *final_vals = nullptr;     // the LAST pass writes its values there instead of into the ping-pong buffer (the initial sort delivers straight into SA this way)
    bool iota = false;                  // value i = index i, vals_in is scratch only
    bool may_skip = false;              // 64-bit keys: look for passes that are the identity (costs a read-back per pass)
    bool first_counted = false;         // the producer of keys_in has histogrammed the first digit (sort_first_counts says where and how)
    int rbits = RADIX_BITS;             // 32-bit keys, 9: nine-bit digits (single-pass engine only, first digit counted by the producer)
    const uint8_t *text = nullptr;      // != nullptr (32-bit keys only; single-pass engine, default tile, counted): the FIRST pass reads its keys from the text (k_onesweep<..., TEXT_KEYS>)
    int64_t text_n = 0;
    int text_bits = 8;                  //   8: the text itself (all 256 byte values), 2: the bit-packed text of a four-symbol alphabet
    int val_extra = 0;                  //   the first pass puts that many key bits below the 32 into the top bits of the values (OnesweepPass::val_extra)
    KeyT *keys_out2 = nullptr;          // != nullptr: keys_in is read-only -- the second pass writes its keys here, not into keys_in
    uint8_t *head_flags = nullptr;      // != nullptr (64-bit keys, single-pass engine, final_vals): the last pass writes `count` group-start flags here and only the keys at
                                        //   the ends of its tiles' digit runs (k_onesweep<..., HEAD_FLAGS>); the rest of the result's keys is then unspecified
    bool poison_keys = false;           // with head_flags: fill that pass's key buffer with 0xA5 bytes first (the diagnostic hook sa_amd_test_sort_pairs_flags)
};
template <typename KeyT>
struct SortResult { KeyT *keys; uint32_t *vals; int passes; int skipped; };

// stats != nullptr: the passes that ran are added to sort_passes and sorted_elements
static int sort_pairs(const SortJob<uint64_t> &j, const SortScratch &ss, hipStream_t st, const Tuning &tn, SortResult<uint64_t> *res, sa_amd_stats *stats = nullptr);
static int sort_pairs32(const SortJob<uint32_t> &j, const SortScratch &ss, hipStream_t st, const Tuning &tn, SortResult<uint32_t> *res, sa_amd_stats *stats = nullptr);
template <typename KeyT>
static void add_passes(sa_amd_stats *stats, const SortResult<KeyT> &res, int64_t count)
{
    if (stats) { stats->sort_passes += res.passes; stats->sorted_elements += (int64_t)res.passes * count; }
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

}  // namespace sa

// The diagnostic library has a second engine (and SA_AMD_NO_ONESWEEP to select it); the product has the single-pass scatter only.
#ifdef SA_AMD_DIAG
#include "sort_diag.hpp"
#else
namespace sa {
constexpr int N_SORT_VARIANTS = 1, N_SORT32_VARIANTS = 1;
static bool three_kernel_engine(const Tuning &) { return false; }
template <typename KeyT>
static int sort_pairs_three_kernel(const SortJob<KeyT> &, const SortScratch &, hipStream_t, const Tuning &, SortResult<KeyT> *)
{
    return SA_AMD_EINTERNAL;        // (no scratch for the single-pass scatter: cannot happen, every caller carves it)
}
template <typename KeyT>
static FirstCounts first_counts_three_kernel(const SortScratch &ss, const Tuning &, int64_t count)
{
    return FirstCounts{ ss.spine, count, 1, ss.spine, (size_t)RADIX * 4 };      // (not reached)
}
}  // namespace sa
#endif

namespace sa {

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

static bool onesweep_on(const SortScratch &ss, const Tuning &tn) { return ss.status != nullptr && !three_kernel_engine(tn); }

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

// the job by the single-pass scatter, one tile shape and digit width; *res: nothing sorted yet
template <typename KeyT, int THREADS, int ITEMS, bool SEQ, int RBITS = RADIX_BITS>
static int sort_pairs_onesweep(const SortJob<KeyT> &j, const SortScratch &ss, hipStream_t st, const Tuning &tn, SortResult<KeyT> *res)
{
    const int64_t count = j.count;
    constexpr int TILE = THREADS * ITEMS;
    constexpr int R = 1 << RBITS;
    static_assert(R <= OS_MAX_RADIX && (RBITS == RADIX_BITS || TILE >= 2 * OS_MIN_TILE), "zones and granule slab are sized for 8-bit digits of 4 Ki-element tiles");
    static_assert(TILE >= OS_MIN_TILE, "the granule slab is sized for tiles of at least OS_MIN_TILE elements");
    constexpr bool K64 = sizeof(KeyT) == 8;
    OnesweepGeom g = onesweep_geom(count, TILE);
    auto zone = [&](int i) { return ss.spine + (size_t)i * OS_ZONE; };
    int z = 0;                                    // zone that holds (or will hold) the counts of the coming pass's digit
    bool have_counts = j.first_counted;
    const int npass = (int)ceil_div(j.end_bit - j.begin_bit, RBITS);
    // every pass's counts up front (k_radix_hist_all): short sorts of keys that exist as an array, no pass to be skipped
    const bool upfront = RBITS == RADIX_BITS && !tn.no_upfront_counts && count < tn.count_next_min_n && !j.may_skip && !j.text && npass <= 8 && npass >= 2;
    if (upfront) { g.nseg = 1; g.tiles_per_seg = g.tiles; g.seg_elems = (int64_t)g.tiles * TILE; }
    HIP_TRY(hipMemsetAsync(ss.status, 0, (size_t)g.tiles * R * 8, st));
    {
        // zone 0 holds the producer's counts (first_counted) and stays; everything behind it starts from zero
        int zones = (j.may_skip ? 2 * npass : npass) + 1;
        if (zones > OS_MAX_ZONES) return SA_AMD_EINTERNAL;
        const int z0 = (j.first_counted && !upfront) ? 1 : 0;      // (up front: the producer counted per segment of another geometry -- counted again)
        HIP_TRY(hipMemsetAsync(zone(z0), 0, (size_t)(zones - z0) * OS_ZONE * 4, st));
    }
    if (upfront) {
        int blocks = (int)ceil_div(count, (int64_t)HA_THREADS * 16);
        if (blocks > 512) blocks = 512;
        if (blocks < 1) blocks = 1;
        PROF(K64 ? KC_UPSWEEP : KC_UPSWEEP32, count, st, hipLaunchKernelGGL((k_radix_hist_all<KeyT>), dim3((unsigned)blocks), dim3(HA_THREADS), 0, st, (const KeyT *)j.keys_in, count,
                                                                        j.begin_bit, j.end_bit, zone(0), (int)OS_ZONE, (int)OS_TICKETS));
        have_counts = true;
    }
    KeyT *kin = j.keys_in, *kout = j.keys_alt;
    uint32_t *vin = j.vals_in, *vout = j.vals_alt;
    constexpr int WG_PER_CU = THREADS <= 512 ? 2 : 1;
    int grid = cu_count() * WG_PER_CU;
    if (grid > g.tiles) grid = g.tiles;
    uint32_t epoch = 0;
    for (int shift = j.begin_bit; shift < j.end_bit; shift += RBITS) {
        const int nb = (j.end_bit - shift) < RBITS ? (j.end_bit - shift) : RBITS;
        const uint32_t dmask = (1u << nb) - 1u;
        const bool last = shift + RBITS >= j.end_bit;
        uint32_t *vdst = (last && j.final_vals) ? j.final_vals : vout;
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
        if (RBITS == RADIX_BITS && j.may_skip && !tn.no_run_skip && count >= tn.run_skip_min && !(j.iota && res->passes == 0) && !(last && j.final_vals)) {
            // a digit that is the same for EVERY element makes the pass the identity (the sort is stable): skip it
            hipLaunchKernelGGL(k_os_digit_totals, dim3(1), dim3(RADIX), 0, st, (const uint32_t *)(zone(z) + OS_TICKETS), g.nseg, ss.digit_tot);
            LAUNCH_CHECK(st);
            uint32_t tot[RADIX];
            { const int rcw = read_words(tot, ss.digit_tot, sizeof(tot), st); if (rcw) return rcw; }
            bool constant = false;
            for (int d = 0; d < RADIX; ++d) constant |= (int64_t)tot[d] == count;
            if (constant) { ++res->skipped; have_counts = false; ++z; continue; }     // (zone z holds the skipped digit's counts: the recount takes the next, clean one)
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
        { const int nbn = (j.end_bit - P.shift_next) < RBITS ? (j.end_bit - P.shift_next) : RBITS; P.dmask_next = last ? 0u : (1u << nbn) - 1u; }
        P.nseg = g.nseg; P.tiles_per_seg = g.tiles_per_seg; P.tiles = g.tiles;
        P.epoch = ++epoch;
        P.flags = (uint32_t)tn.onesweep_flags;
        P.text = j.text; P.text_n = j.text_n; P.text_bits = j.text_bits;
        P.val_extra = (j.text && res->passes == 0 && j.iota) ? j.val_extra : 0;
        // (the flags pass exists for 64-bit keys only: a 32-bit sort ignores head_flags, and so does every pass but the last)
        constexpr bool FLAGS_OK = K64 && RBITS == RADIX_BITS;
        P.head_flags = (FLAGS_OK && last && j.final_vals) ? j.head_flags : nullptr;
        if (P.head_flags) {
            if constexpr (FLAGS_OK) {
                if (j.poison_keys) HIP_TRY(hipMemsetAsync(kout, 0xA5, (size_t)count * sizeof(KeyT), st));
                PROF(KC_ONESWEEP, count, st,
                     hipLaunchKernelGGL((k_onesweep<THREADS, ITEMS, KeyT, SEQ, WG_PER_CU, RBITS, false, true>), dim3(grid), dim3(THREADS), 0, st, (const KeyT *)kin,
                                        (const uint32_t *)((j.iota && res->passes == 0) ? nullptr : vin), kout, vdst, P));
            }
        } else if (!K64 && !SEQ && j.text && res->passes == 0)
            PROF(KC_ONESWEEP32, count, st,
                 hipLaunchKernelGGL((k_onesweep<THREADS, ITEMS, KeyT, SEQ, WG_PER_CU, RBITS, !K64 && !SEQ>), dim3(grid), dim3(THREADS), 0, st, (const KeyT *)kin,
                                    (const uint32_t *)((j.iota && res->passes == 0) ? nullptr : vin), kout, vdst, P));
        else
        PROF(K64 ? KC_ONESWEEP : KC_ONESWEEP32, count, st,
             hipLaunchKernelGGL((k_onesweep<THREADS, ITEMS, KeyT, SEQ, WG_PER_CU, RBITS>), dim3(grid), dim3(THREADS), 0, st, (const KeyT *)kin,
                                (const uint32_t *)((j.iota && res->passes == 0) ? nullptr : vin), kout, vdst, P));
        KeyT *tk = kin; kin = kout; kout = (j.keys_out2 && res->passes == 0) ? j.keys_out2 : tk;
        uint32_t *free_v = vin;                   // the values just consumed become the next scratch target
        vin = vdst;
        vout = free_v;
        ++res->passes;
        ++z;
        have_counts = count_next || upfront;
    }
    res->keys = kin; res->vals = vin;
    return SA_AMD_OK;
}

static int sort_pairs(const SortJob<uint64_t> &j, const SortScratch &ss, hipStream_t st, const Tuning &tn, SortResult<uint64_t> *res, sa_amd_stats *stats)
{
    *res = SortResult<uint64_t>{ j.keys_in, j.vals_in, 0, 0 };
    if (j.count <= 1 || j.end_bit <= j.begin_bit) return SA_AMD_OK;
    int rc;
    if (!onesweep_on(ss, tn)) rc = sort_pairs_three_kernel(j, ss, st, tn, res);
    else switch (tn.onesweep64_shape) {
        case 1: rc = sort_pairs_onesweep<uint64_t, 512, 16, true>(j, ss, st, tn, res); break;
        case 2: rc = sort_pairs_onesweep<uint64_t, 512, 8, false>(j, ss, st, tn, res); break;
        default: rc = sort_pairs_onesweep<uint64_t, 1024, 8, false>(j, ss, st, tn, res); break;
    }
    if (rc == SA_AMD_OK) add_passes(stats, *res, j.count);
    return rc;
}

static int sort_pairs32(const SortJob<uint32_t> &j, const SortScratch &ss, hipStream_t st, const Tuning &tn, SortResult<uint32_t> *res, sa_amd_stats *stats)
{
    *res = SortResult<uint32_t>{ j.keys_in, j.vals_in, 0, 0 };
    if (j.may_skip) return SA_AMD_EINTERNAL;       // (no 32-bit sort looks for identity passes)
    if (j.keys_out2 && (j.rbits != RADIX_BITS || j.text)) return SA_AMD_EINTERNAL;
    if (j.count <= 1 || j.end_bit <= j.begin_bit) return SA_AMD_OK;
    if (j.rbits != RADIX_BITS && (j.rbits != 9 || !onesweep_on(ss, tn) || !j.first_counted)) return SA_AMD_EINTERNAL;
    if (j.text && (!onesweep_on(ss, tn) || !j.first_counted || tn.onesweep32_shape != 0)) return SA_AMD_EINTERNAL;
    int rc;
    if (!onesweep_on(ss, tn)) rc = sort_pairs_three_kernel(j, ss, st, tn, res);
    else if (j.rbits == 9) rc = sort_pairs_onesweep<uint32_t, 1024, 12, false, 9>(j, ss, st, tn, res);
    else if (j.text) rc = sort_pairs_onesweep<uint32_t, 1024, 12, false>(j, ss, st, tn, res);
    else switch (tn.onesweep32_shape) {
        case 1: rc = sort_pairs_onesweep<uint32_t, 512, 16, true>(j, ss, st, tn, res); break;
        case 2: rc = sort_pairs_onesweep<uint32_t, 512, 12, false>(j, ss, st, tn, res); break;
        case 3: rc = sort_pairs_onesweep<uint32_t, 1024, 8, false>(j, ss, st, tn, res); break;
        default: rc = sort_pairs_onesweep<uint32_t, 1024, 12, false>(j, ss, st, tn, res); break;
    }
    if (rc == SA_AMD_OK) add_passes(stats, *res, j.count);
    return rc;
}

static FirstCounts sort_first_counts(const SortScratch &ss, const Tuning &tn, int64_t count, bool keys32)
{
    if (!onesweep_on(ss, tn)) return keys32 ? first_counts_three_kernel<uint32_t>(ss, tn, count) : first_counts_three_kernel<uint64_t>(ss, tn, count);
    FirstCounts f;
    const OsShape &sh = keys32 ? os_shapes32[tn.onesweep32_shape] : os_shapes64[tn.onesweep64_shape];
    const int tile = sh.threads * sh.items;
    const OnesweepGeom g = onesweep_geom(count, tile);
    f.counts = ss.spine + OS_TICKETS; f.chunk_elems = g.seg_elems; f.G = g.nseg;
    f.zero_ptr = ss.spine; f.zero_bytes = (size_t)OS_ZONE * 4;
    return f;
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

}  // namespace sa
