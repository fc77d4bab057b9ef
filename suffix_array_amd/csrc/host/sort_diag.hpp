// host/sort_diag.hpp -- DIAGNOSTIC LIBRARY ONLY (-DSA_AMD_DIAG), included by host/sort.hpp: the second sort engine, the three-kernel
// pass of rounds 1-2 (kernels/radix_sort_diag.hpp; SA_AMD_NO_ONESWEEP=1 / SA_AMD_SORT_VARIANT / SA_AMD_SORT32_VARIANT select it for A/B
// measurements and for the primitive tests that compare the two engines), and the sample sort of the 64-bit stage (sample_sort64).
// Included by host/sort.hpp, behind the job, result and scratch types and in front of the drivers.
#pragma once

namespace sa {

static bool three_kernel_engine(const Tuning &tn) { return tn.no_onesweep; }

// Tile-scatter kernel shapes (threads, items per thread, workgroups per CU).  SA_AMD_SORT_VARIANT selects one at run
// time for A/B measurements; the first four sort correctly.  Behind them come the first-generation scatter, its timing
// ablations (wrong orders, on purpose) and the phase-stamp build.
template <typename KeyT>
using DownsweepFn = void (*)(const KeyT *, const uint32_t *, KeyT *, uint32_t *, uint32_t *, const uint32_t *, int64_t, int, uint32_t, int64_t, int);
struct SortVariant { int threads, items, wg_per_cu; DownsweepFn<uint64_t> fn; const char *name; };
static const SortVariant sort_variants[] = {
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8, 16, 1, false, uint64_t, 4>, "carry-completed lines 1024x8 + LDS prefetch of half of the next tile's keys (default)" },
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8>, "carry-completed lines 1024x8" },
    { 512, 16, 1, k_radix_downsweep_wcl<512, 16>, "carry-completed lines 512x16" },
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8, 8>, "carry 1024x8, granule 8" },
    // (two workgroups per CU at 64 VGPRs -- 1024x4 or 512x8 with granule 8 -- measured slower: C3-iid 28.0 -> 29.8 .. 33.9 ms)
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4>, "plain tile scatter 1024x8 (first generation)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 1>, "plain 1024x8 ABLATION sequential stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 33>, "plain 1024x8 ABLATION no ranking + sequential stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 16>, "plain 1024x8 ABLATION no stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep<1024, 8, 4, 49>, "plain 1024x8 ABLATION no ranking, no stores (wrong results)" },
    { 1024, 8, 2, k_radix_downsweep_wcl<1024, 8, 16, 1, true>, "carry 1024x8 DIAGNOSTIC phase stamps (tools/phase_stamps.py)" },
};
constexpr int N_SORT_VARIANTS = (int)(sizeof(sort_variants) / sizeof(sort_variants[0]));

// 32-bit keys (two-stage initial sort): same three-kernel pass, 12 Ki-pair tiles by default (the LDS stage holds more 4-byte elements)
constexpr int SORT32_THREADS = 1024;
struct Sort32Variant { int items; DownsweepFn<uint32_t> fn; };
static const Sort32Variant sort32_variants[] = {
    { 12, k_radix_downsweep_wcl<SORT32_THREADS, 12, 16, 1, false, uint32_t, 12> },    // default: next tile's keys prefetched into LDS
    { 12, k_radix_downsweep_wcl<SORT32_THREADS, 12, 16, 1, false, uint32_t> },
    { 8, k_radix_downsweep_wcl<SORT32_THREADS, 8, 16, 1, false, uint32_t> },
    { 16, k_radix_downsweep_wcl<SORT32_THREADS, 16, 16, 1, false, uint32_t> },        // spills
    { 8, k_radix_downsweep_wcl<SORT32_THREADS, 8, 16, 1, false, uint32_t, 8> },
    // (two workgroups per CU: 1024 x 4 or 1024 x 8 with granule 8 and 64 VGPRs measured slower, 8.6 -> 9.0 .. 10.2 ms at 256 MiB)
};
constexpr int N_SORT32_VARIANTS = (int)(sizeof(sort32_variants) / sizeof(sort32_variants[0]));

struct SortGrid { int G; int64_t tiles_per_wg, tile; int threads; };
static SortGrid sort_grid(int64_t count, const SortVariant &sv)
{
    SortGrid g;
    g.tile = sv.threads * sv.items;
    g.threads = sv.threads;
    const int64_t tiles = ceil_div(count, g.tile);
    int max_wg = 256 * sv.wg_per_cu;
    if (max_wg > SORT_MAX_WG) max_wg = SORT_MAX_WG;
    g.tiles_per_wg = ceil_div(tiles, max_wg);
    if (g.tiles_per_wg < 1) g.tiles_per_wg = 1;
    g.G = (int)ceil_div(tiles, g.tiles_per_wg);
    if (g.G < 1) g.G = 1;
    return g;
}
static SortGrid sort_grid(int64_t count, const Sort32Variant &sv)
{
    SortGrid g;
    g.tile = (int64_t)SORT32_THREADS * sv.items;
    g.threads = SORT32_THREADS;
    const int64_t tiles = ceil_div(count, g.tile);
    g.tiles_per_wg = ceil_div(tiles, 512);
    if (g.tiles_per_wg < 1) g.tiles_per_wg = 1;
    g.G = (int)ceil_div(tiles, g.tiles_per_wg);
    return g;
}

// what the pass of the two key widths does not share: the shape table, the counting kernel and how its parts are cut
template <typename KeyT> struct ThreeKernel;
template <> struct ThreeKernel<uint64_t> {
    static constexpr KClass UPSWEEP = KC_UPSWEEP, DOWNSWEEP = KC_DOWNSWEEP;
    static constexpr int64_t PART_MIN = 4096, PART_ALIGN = 2;      // smallest part of a chunk, keys per 16-byte load
    static constexpr auto upsweep = k_radix_upsweep;
    static const SortVariant &variant(const Tuning &tn) { return sort_variants[tn.sort_variant]; }
};
template <> struct ThreeKernel<uint32_t> {
    static constexpr KClass UPSWEEP = KC_UPSWEEP32, DOWNSWEEP = KC_DOWNSWEEP32;
    static constexpr int64_t PART_MIN = 8192, PART_ALIGN = 4;
    static constexpr auto upsweep = k_radix_upsweep32;
    static const Sort32Variant &variant(const Tuning &tn) { return sort32_variants[tn.sort32_variant]; }
};

// the job of sort_pairs / sort_pairs32 by the three-kernel pass; spine: per-chunk counts, RADIX * G words
template <typename KeyT>
static int sort_pairs_three_kernel(const SortJob<KeyT> &j, const SortScratch &ss, hipStream_t st, const Tuning &tn, SortResult<KeyT> *res)
{
    using E = ThreeKernel<KeyT>;
    const int64_t count = j.count;
    uint32_t *spine = ss.spine, *digit_tot = ss.digit_tot;
    const auto &sv = E::variant(tn);
    const SortGrid g = sort_grid(count, sv);
    KeyT *kin = j.keys_in, *kout = j.keys_alt;
    uint32_t *vin = j.vals_in, *vout = j.vals_alt;
    for (int shift = j.begin_bit; shift < j.end_bit; shift += RADIX_BITS) {
        const int nb = (j.end_bit - shift) < RADIX_BITS ? (j.end_bit - shift) : RADIX_BITS;
        const uint32_t dmask = (1u << nb) - 1u;
        const bool last = shift + RADIX_BITS >= j.end_bit;
        uint32_t *vdst = (last && j.final_vals) ? j.final_vals : vout;
        {
            const int64_t chunk = g.tiles_per_wg * g.tile;
            int split = 2048 / g.G;
            if (split < 1) split = 1;
            while (split > 1 && chunk / split < E::PART_MIN) split /= 2;
            const int64_t sub = (ceil_div(chunk, split) + E::PART_ALIGN - 1) & ~(E::PART_ALIGN - 1);
            // (atomic accumulation needs a zeroed spine: once here, afterwards every downsweep zeroes what it consumed)
            if (j.first_counted && shift == j.begin_bit) {
                // (nothing to do: k_build_keys has added this pass's digit counts to the spine)
            } else {
                if (split > 1 && res->passes == 0) HIP_TRY(hipMemsetAsync(spine, 0, (size_t)RADIX * g.G * 4, st));
                PROF(E::UPSWEEP, count, st, hipLaunchKernelGGL((E::upsweep), dim3(g.G * split), dim3(SORT_THREADS), 0, st, (const KeyT *)kin, spine,
                                                               count, shift, dmask, chunk, g.G, split, sub));
            }
        }
        PROF(KC_SPINE, (int64_t)RADIX * g.G, st, hipLaunchKernelGGL((k_spine_rows), dim3(RADIX), dim3(SPINE_THREADS), 0, st,
                                                                    spine, digit_tot, g.G));
        // A digit that is the same for EVERY element makes the pass the identity (the sort is stable): skip the tile scatter.
        // Worth a 1 KiB read-back (a host round trip of ~30 us) only for the large global sorts of the refinement rounds: texts
        // that are one run or one period keep hundreds of millions of suffixes in a few groups round after round, and their
        // (group, rank) keys are constant in most digits.  The ISA passes never look, the initial sort only for a text of one byte value.
        if (j.may_skip && !tn.no_run_skip && count >= tn.run_skip_min && !(j.iota && res->passes == 0) && !(last && j.final_vals)) {
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
        PROF(E::DOWNSWEEP, count, st, hipLaunchKernelGGL((sv.fn), dim3(g.G), dim3(g.threads), 0, st,
                                                         (const KeyT *)kin, (const uint32_t *)((j.iota && res->passes == 0) ? nullptr : vin), kout, vdst,
                                                         spine, (const uint32_t *)digit_tot, count, shift,
                                                         dmask, g.tiles_per_wg, g.G));
        KeyT *tk = kin; kin = kout; kout = (j.keys_out2 && res->passes == 0) ? j.keys_out2 : tk;
        uint32_t *free_v = vin;     // the values just consumed become the next scratch target
        vin = vdst;
        vout = free_v;
        res->passes++;
    }
    res->keys = kin; res->vals = vin;
    return SA_AMD_OK;
}

// sort_first_counts for this engine: the producer's counts go straight into the spine
template <typename KeyT>
static FirstCounts first_counts_three_kernel(const SortScratch &ss, const Tuning &tn, int64_t count)
{
    FirstCounts f;
    const SortGrid g = sort_grid(count, ThreeKernel<KeyT>::variant(tn));
    f.counts = ss.spine; f.zero_ptr = ss.spine;
    f.chunk_elems = g.tiles_per_wg * g.tile; f.G = g.G;
    f.zero_bytes = (size_t)RADIX * f.G * 4;
    return f;
}

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
    SortJob<uint64_t> sj{ samp, u0, samp_alt, u1, S, 0, key_bits };
    sj.iota = true;
    SortResult<uint64_t> sr;
    int rc = sort_pairs(sj, ss, st, tn, &sr, local);
    if (rc) return rc;
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

}  // namespace sa
