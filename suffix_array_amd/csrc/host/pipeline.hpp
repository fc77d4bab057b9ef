// host/pipeline.hpp -- the device pipeline of one build: workspace layout, refinement rounds, build_device().  The radix-sort
// drivers are in host/sort.hpp, the posted read-back (read_words) in host/readback.hpp.
// Replaces the arithmetic behind `cdivsufsort::sort_in_place` (reference src/saca.rs:14).
// There is deliberately no CPU fallback: every step launches the HIP kernels of kernels/*.hpp or returns an error code.
#pragma once
#include "support.hpp"
#include "tuning.hpp"
#include "pool.hpp"
#include "sort.hpp"
#include "readback.hpp"

#include <algorithm>
#include <functional>

namespace sa {

// The tuning of one call, read from the environment: the one place that passes the engines' variant counts (host/sort.hpp).
static inline Tuning env_tuning() { return Tuning::from_env(N_SORT_VARIANTS, N_SORT32_VARIANTS, N_OS_SHAPES64, N_OS_SHAPES32); }
// The same for a route that reads words back (read_words): the calling thread's posted read-backs follow the tuning.
static inline Tuning route_tuning()
{
    const Tuning tn = env_tuning();
    g_posted_off = tn.no_posted_readback;
    return tn;
}

constexpr size_t GRAM_MAX_ENTRIES = (size_t)1 << 24;   // gram keys: the rank table has sigma^g <= min(n, 2^24) entries
static_assert(GROUP_CAP_MAX == GS_CAP, "Tuning clamps SA_AMD_GROUP_CAP to the kernel's cap");

// device scratch layout for a text of n bytes
struct Workspace {
    uint64_t *keysA, *keysB, *keysC;
    uint32_t *valsA, *valsB, *isa, *U0, *U1, *G0, *G1;
    uint32_t *tcnt, *thead, *tnext, *hist, *total, *chg, *has_isa;
    uint8_t *packed;           // bit-packed text (alphabets of 2, 4 or 16 symbols): n / 2 + 64 bytes
    uint8_t *gram_flags;       // gram keys: which g-grams occur (sigma^g <= min(n, 2^24) flags) and
    uint4 *gram_table;         //   the rank directory over them (16 bytes per 64 indices)
    uint32_t *surv_bits, *surv_cnt, *todo_bits, *ft_cnt, *ft_head;   // first refinement round straight from the sorted keys (k_finish_sorted)
    uint32_t *bk_start;             // bucket sort of the 32-bit first stage: 2^16 + 1 or 2^18 + 1 bucket starts
    uint32_t *early_bits, *early_cnt;    // early download: bitmap over the n + 1 entries of the downloaded array, marked entries per tile
    SortScratch ss;                 // spine, digit totals and look-back granules of the radix sorts (2 KiB per 8192-element tile); ss.err: 64 words, the
                                    //   sorts' give-ups in word 0, the bucket sort's two words from word 2
    size_t bytes, bytes2;           // in the first (device) block, in the second (reduced-memory route: pinned host) block
};

// Slabs are laid out in the order of the take() calls below.  cap / base2: the REDUCED-MEMORY route of the host-pointer entry
// points (host/host_path.hpp): when the device cannot give the whole workspace, the first `cap` bytes' worth of slabs live in
// the device block `base` and every slab that no longer fits lives in `base2`, a block of pinned host memory that the kernels
// reach over PCIe (slow, correct: the alternative is SA_AMD_ENOMEM).  So the order below is by need: first the small slabs that
// workgroups talk through (look-back granules, tickets, counters -- they must be device memory), then the big ones from the most
// to the least used.  w.bytes = bytes in the first block, w.bytes2 = bytes in the second (0 without a cap).
static Workspace carve(void *base, int64_t n, size_t cap = ~(size_t)0, void *base2 = nullptr)
{
    Workspace w;
    const size_t N = (size_t)(n > 0 ? n : 1);
    size_t off = 0, off2 = 0;
    auto take = [&](size_t b) {
        if (off + b <= cap) { size_t o = off; off = align_up(off + b, 256); return (char *)base + o; }
        size_t o = off2; off2 = align_up(off2 + b, 256); return (char *)base2 + o;
    };
    const size_t rr_tiles = (size_t)ceil_div((int64_t)N, RR_TILE);
    const size_t ft_tiles = (size_t)ceil_div((int64_t)N, FT_TILE) + 1;
    const size_t gram_entries = N < GRAM_MAX_ENTRIES ? N : GRAM_MAX_ENTRIES;
    // ---- small, shared between workgroups ----
    {
        void *spine = take(SortScratch::SPINE_BYTES), *granules = take(SortScratch::granule_bytes((int64_t)N));
        w.ss = SortScratch::make(spine, granules, (uint32_t *)take(256));
    }
    w.hist = (uint32_t *)take(256 * 4);
    w.total = (uint32_t *)take(256);
    w.chg = (uint32_t *)take((size_t)RR_CHG_COUNTERS * 32 * 4);      // (directly behind w.total: read back together)
    w.tcnt = (uint32_t *)take(rr_tiles * 4);
    w.thead = (uint32_t *)take(rr_tiles * 4);
    w.tnext = (uint32_t *)take(rr_tiles * 4);
    w.surv_cnt = (uint32_t *)take(rr_tiles * 4);          // (not tcnt: a refinement round uses that one for its own compaction)
    w.ft_cnt = (uint32_t *)take(ft_tiles * 4);
    w.ft_head = (uint32_t *)take(ft_tiles * 4);
    w.bk_start = (uint32_t *)take(((size_t)BK_BUCKETS_MAX + 1) * 4);
    w.early_cnt = (uint32_t *)take(((N + 1 + EARLY_TILE - 1) / EARLY_TILE + 8) * 4);
    w.gram_table = (uint4 *)take((gram_entries / 64 + 1) * 16);
    // ---- n / 8 .. n / 2 bytes ----
    w.has_isa = (uint32_t *)take((N + 31) / 32 * 4);
    w.surv_bits = (uint32_t *)take((N + 31) / 32 * 4);
    w.todo_bits = (uint32_t *)take((N + 31) / 32 * 4);
    w.early_bits = (uint32_t *)take(((N + 1 + 31) / 32 + EARLY_THREADS) * 4);           // (whole tiles of 256 words)
    w.gram_flags = (uint8_t *)take(gram_entries + 64);
    w.packed = (uint8_t *)take(N / 2 + 64);
    // ---- the big ones, most used first ----
    w.keysA = (uint64_t *)take((N + 64) * 8);         // (+64: as two halves of n + 1 32-bit entries each, see scatter_binned)
    w.keysB = (uint64_t *)take((N + 64) * 8);
    w.valsA = (uint32_t *)take(N * 4);
    w.valsB = (uint32_t *)take(N * 4);
    w.isa = (uint32_t *)take(N * 4);
    w.U0 = (uint32_t *)take(N * 4);
    w.G0 = (uint32_t *)take(N * 4);
    w.U1 = (uint32_t *)take(N * 4);
    w.G1 = (uint32_t *)take(N * 4);
    w.keysC = (uint64_t *)take((N + 64) * 8);
    w.bytes = off;
    w.bytes2 = off2;
    return w;
}

// symbol codes and key geometry from the sigma = 256 histogram; returns the number of key bits to sort
static int make_key_params(const uint32_t *hist, KeyParams *P, int *sigma_out, int kb_max = 64)
{
    int sigma = 0;
    for (int c = 0; c < 256; ++c) {
        if (hist[c]) P->code[c] = (uint8_t)sigma++;
        else P->code[c] = 0;
    }
    *sigma_out = sigma;
    P->packed = nullptr;
    P->gram = 0; P->gram_m = 0; P->gram_tail = 0; P->gram_top = 0; P->gram_D = 0; P->gram_table = nullptr;
    const uint64_t se = sigma > 2 ? (uint64_t)sigma : 2u;      // effective radix (a unary text still needs one bit)
    P->sigma = se;
    // kb_max < 64 (A/B): fewer key bits = fewer radix passes, more left to the rounds
    if ((se & (se - 1)) == 0) {                                // power of two: plain bit fields
        const int bits = bit_length(se - 1);
        P->bits = bits;
        P->k = kb_max / bits;
        const int used = P->k * bits;
        P->mask = used >= 64 ? ~0ull : ((1ull << used) - 1ull);
        P->top = 0;
        return used;
    }
    // otherwise pack as a base-sigma number: the largest k with sigma^k <= 2^64
    unsigned __int128 pw = 1;
    int k = 0;
    while (pw * se <= ((unsigned __int128)1 << kb_max)) { pw *= se; ++k; }
    P->bits = 0;
    P->k = k;
    P->mask = ~0ull;
    uint64_t top = 1;
    for (int i = 0; i + 1 < k; ++i) top *= se;
    P->top = top;
    const unsigned __int128 maxkey = pw - 1;                   // fits in 64 bits
    return bit_length((uint64_t)maxkey);
}

// Binned ISA writes (one radix pass on the top bits of the suffix position, then a windowed scatter) pay off once the ISA is
// far larger than the caches: always for the full build (n entries), for a round's update only when it rewrites at least
// binned_min entries (measured on C3: direct stores of the CHANGED ranks win below 64 M pairs)
static bool binned(int64_t n, int64_t count, const Tuning &tn)
{
    if (tn.no_binned_isa) return false;
    if (tn.binned_isa_always) return count > 0;      // tests: exercise the path at small sizes
    return n >= ((int64_t)1 << 25) && (count >= n || count >= tn.binned_min);
}

// (suffix, rank) pairs (both 32 bits) -> ISA.  Large batches: two radix passes on the top 16 bits of the suffix position, then
// windows of the ISA are assembled in LDS and stored in address order (k_scatter_windows); smaller ones: one pass on the top
// 8 bits and a plain scatter inside 2^(nb-8)-entry windows.  SA_AMD_SCATTER_LEVELS = 1 / 2 forces either.
// iota: the value of pair i is i and pk is READ-ONLY (the suffix array itself): the passes then go pk -> (altk, altv) ->
// (altk2, altv2) and never write into pk.  Without iota, altk2 != nullptr: pk is read-only likewise (the keys of the rank set-up
// are the suffix array), the second pass writes its keys to altk2 and its values back into pv.
static int scatter_binned(const SortScratch &ss, uint32_t *isa, uint32_t *pk, uint32_t *pv, uint32_t *altk, uint32_t *altv, int64_t count, int64_t n,
                          hipStream_t st, sa_amd_stats *local, const Tuning &tn, bool iota = false,
                          uint32_t *altk2 = nullptr, uint32_t *altv2 = nullptr)
{
    const int nb = bit_length((uint64_t)(n > 1 ? n : 1));          // (the sentinel value n may be among the keys)
    int wlog = nb - 16;                                              // window = 2^wlog ISA entries, assembled in LDS
    if (wlog < 10) wlog = 10;                                        // small texts: one pass covers the bits above the window
    if (wlog > 15) wlog = 15;                                        // (n < 2^31, so nb <= 31)
    // (a text of fewer than 2^10 bytes has no bits above the window: the one-pass form below does it)
    const bool two = nb > wlog && (tn.scatter_levels == 2 || (tn.scatter_levels == 0 && count >= ((int64_t)1 << 25)));
    SortResult<uint32_t> pr;
    if (two) {
        int rc;
        if (iota) {
            const int mid = wlog + RADIX_BITS < nb ? wlog + RADIX_BITS : nb;
            SortJob<uint32_t> first{ pk, nullptr, altk, altv, count, wlog, mid };
            first.iota = true;
            rc = sort_pairs32(first, ss, st, tn, &pr, local);
            if (rc) return rc;
            if (pr.passes != 1) return SA_AMD_EINTERNAL;            // (cannot happen: nb > wlog whenever count > 1)
            if (mid < nb) {
                rc = sort_pairs32(SortJob<uint32_t>{ altk, altv, altk2, altv2, count, mid, nb }, ss, st, tn, &pr, local);
                if (rc) return rc;
            }
        } else {
            SortJob<uint32_t> both{ pk, pv, altk, altv, count, wlog, nb };
            both.keys_out2 = altk2;
            rc = sort_pairs32(both, ss, st, tn, &pr, local);
            if (rc) return rc;
        }
        const unsigned grid = (unsigned)ceil_div(count, SW_CHUNK);
        if (wlog <= 13)
            PROF(KC_SCATTER, count, st, hipLaunchKernelGGL((k_scatter_windows<13>), dim3(grid), dim3(SW_THREADS), 0, st, (const uint32_t *)pr.keys,
                                                           (const uint32_t *)pr.vals, isa, count, (uint32_t)n, wlog));
        else
            PROF(KC_SCATTER, count, st, hipLaunchKernelGGL((k_scatter_windows<15>), dim3(grid), dim3(SW_THREADS), 0, st, (const uint32_t *)pr.keys,
                                                           (const uint32_t *)pr.vals, isa, count, (uint32_t)n, wlog));
        return SA_AMD_OK;
    }
    const int shift = nb > RADIX_BITS ? nb - RADIX_BITS : 0;
    SortJob<uint32_t> one{ pk, pv, altk, altv, count, shift, shift + RADIX_BITS };
    one.iota = iota;
    const int rc = sort_pairs32(one, ss, st, tn, &pr, local);
    if (rc) return rc;
    PROF(KC_SCATTER, count, st, hipLaunchKernelGGL((k_scatter_pairs<uint32_t>), dim3((unsigned)ceil_div(count, 1024)), dim3(256), 0, st,
                                                   (const uint32_t *)pr.keys, (const uint32_t *)pr.vals, isa, count, (uint32_t)n));
    return SA_AMD_OK;
}

}  // namespace sa
#include "refine_round.hpp"      // a refinement round and what it works on (BuildCore); uses Workspace and scatter_binned above
namespace sa {

// Gram keys: how many of the sigma^g possible g-grams occur?  A word-structured text uses a small part of them, so a key of
// dense gram ranks holds more symbols than the base-sigma form, often in fewer digits (C3, sigma = 57: 12 symbols in 7
// passes instead of 10 in 8).  Measured (flags, count, scan), then decided: *P and *key_bits change only when the gram form
// holds more symbols, or as many in fewer radix passes.
static int choose_gram_keys(const uint8_t *dT, int64_t n, KeyParams *Pp, int *key_bits, const Workspace &w, hipStream_t st,
                            const Tuning &tn, bool trace)
{
    KeyParams &P = *Pp;
    const uint64_t se = P.sigma;
    const uint64_t cap = (uint64_t)((size_t)n < GRAM_MAX_ENTRIES ? (size_t)n : GRAM_MAX_ENTRIES);
    int g = 0;
    uint64_t S = 1;
    for (int t = 1; t <= 8; ++t) {
        if (S * se > cap) break;
        S *= se; g = t;
        if (tn.gram_g >= 2 && g == tn.gram_g) break;
    }
    if (g < 2) return SA_AMD_OK;
    uint64_t top = 1;
    for (int t = 0; t + 1 < g; ++t) top *= se;
    const int64_t gtiles = ceil_div((int64_t)S, GT_TILE);
    HIP_TRY(hipMemsetAsync(w.gram_flags, 0, (size_t)S, st));
    PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_gram_mark), dim3((unsigned)ceil_div(ceil_div(n, KB_TILE), GM_TPW)), dim3(KB_THREADS), 0, st, dT, n, P, g,
                                            (uint32_t)top, w.gram_flags));
    PROF(KC_MISC, (int64_t)S, st, hipLaunchKernelGGL((k_gram_count), dim3((unsigned)gtiles), dim3(GT_THREADS), 0, st,
                                            (const uint8_t *)w.gram_flags, (int64_t)S, w.tcnt));
    PROF(KC_RR_SCAN, gtiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, gtiles, w.total));
    uint32_t D = 0;
    { const int rcw = read_words(&D, w.total, 4, st); if (rcw) return rcw; }
    int m = 0;
    unsigned __int128 pw = 1;
    while (D >= 2 && (m + 1) * g <= 64 && pw * D <= ((unsigned __int128)1 << 64)) { pw *= D; ++m; }
    // the bits a whole further gram does not fit into take plain symbols (base-sigma digits behind the gram ranks): C3's
    // 3 four-grams leave 9.7 of the 64 bits idle, one symbol of 5.8 bits makes the key 13 symbols deep for one more pass
    int tail = 0;
    while (m > 0 && tail < tn.gram_tail_max && m * g + tail + 1 <= 64 && pw * se <= ((unsigned __int128)1 << 64)) { pw *= se; ++tail; }
    const int gram_bits = m > 0 ? bit_length((uint64_t)(pw - 1)) : 0;
    const int plain_passes = (int)ceil_div(*key_bits, RADIX_BITS), gram_passes = (int)ceil_div(gram_bits, RADIX_BITS);
    const int syms = m * g + tail;
    const bool better = m > 0 && (syms > P.k || (syms == P.k && gram_passes < plain_passes));
    if (trace) fprintf(stderr, "suffix_array_amd: gram keys: %u of %llu %d-grams occur -> %d symbols (%d grams + %d plain) in %d bits (plain: %d in %d) -> %s\n",
                       D, (unsigned long long)S, g, syms, m, tail, gram_bits, P.k, *key_bits, better ? "gram keys" : "plain keys");
    if (!better) return SA_AMD_OK;
    PROF(KC_MISC, (int64_t)S, st, hipLaunchKernelGGL((k_gram_table), dim3((unsigned)gtiles), dim3(GT_THREADS), 0, st,
                                            (const uint8_t *)w.gram_flags, (int64_t)S, (const uint32_t *)w.tcnt, w.gram_table));
    P.gram = g; P.gram_m = m; P.gram_tail = tail; P.gram_top = (uint32_t)top; P.gram_D = D; P.gram_table = w.gram_table;
    P.bits = 0; P.k = syms; P.mask = ~0ull;
    *key_bits = gram_bits;
    return SA_AMD_OK;
}

// Early download (host/host_path.hpp): what the host-pointer entry points hand to the build so that the suffix array can start
// its way over PCIe while the last refinement rounds run.  The build calls start() once, when the tied list has come down to
// `threshold` suffixes -- by then it has marked the snapshot of the tied slots (k_early_mark) and written SA[0] --, and stop()
// when the rounds are done; stop() returns how many entries of the array (from its front) were or are being copied, and the
// build compacts the final values of the marked entries among them (d_holes, in entry order; d_tile_off = where each tile of
// EARLY_TILE entries starts in d_holes; d_bits = the marks).
struct EarlyDownload {
    int off = 0;                          // in: entry of slot 0 in the downloaded array (1: the array starts with the sentinel entry SA[0] = n)
    int64_t threshold = 0;                // in: start when at most this many suffixes are tied (0: never)
    std::function<void(hipEvent_t)> start;   // in: begin copying the array from its front; the copy stream must wait for the event first
    std::function<int64_t()> stop;        // in: no further chunk is started; returns the entries [0, x) that were handed to the copy
    bool started = false;
    int64_t m_snap = 0;                   // out: tied suffixes at the snapshot
    int64_t covered = 0;                  // out: stop()'s answer
    int64_t holes = 0;                    // out: marked entries among the covered ones
    const uint32_t *d_bits = nullptr, *d_tile_off = nullptr, *d_holes = nullptr;      // out (device pointers into the workspace)
    hipEvent_t ev = nullptr;
};

// What is decided before the first key is built: geometry_and_probes fills it, every later phase reads it (const).  g_bits, the
// bits of a slot, is part of the geometry too and stays in BuildCore, where the rounds read it.
struct Route {
    KeyParams P, Pp;                    // the key geometry, plain or gram form; Pp: the same with the bit-packed text (w.packed, != nullptr: initial_sort
                                        //   writes it) -- every launch behind the key building takes Pp, the key building itself and the probes P
    int sigma = 0, key_bits = 0, top_shift = 0;      // top_shift != 0: 32-bit first stage on the key bits from there up
    int bucket_top_bits = 0;            // ... key bits its two global passes in front of the bucket sort order, first estimate (0: four global passes)
    bool flat_text = false;             // short text whose byte values are equally frequent: narrower initial keys
    bool unary = false;                 // a text of one byte value: the array was written directly, nothing else runs
    bool force_dense = false, text_ok = false, probe_dense = false;
    bool dense_expected() const { return force_dense || probe_dense || !text_ok; }      // rank doubling right behind the initial sort
};
// What initial_sort leaves: SA holds the suffixes in the order of their initial keys
struct InitialOrder {
    SortResult<uint64_t> sr;            // sr.keys: the initial keys in SA order (kept for the rank look-ups); 32-bit stage: the 8n-byte buffer of `sorted32`
    const uint32_t *sorted32 = nullptr; // 32-bit stage: the sorted 32-bit keys (no 64-bit sorted array exists)
    bool bucket_finished = false;       // ... and k_bucket_sort has already ordered the suffixes tied on those 32 bits by their low key bits
    // Group-start flags (kernels/common.hpp, OS_HF_*): != nullptr: the last pass of the 64-bit initial sort wrote one flag byte per slot
    // here instead of the sorted keys, and sr.keys holds true keys only at the ends of that pass's digit runs.  The first re-rank
    // (group_heads, the rank set-up of the dense route) reads the flags; every other reader of the sorted keys gets them rebuilt first
    // (rebuild_sorted_keys).  They live in w.keysC, which nothing else touches between the last sort pass and the end of the first k_rr_apply.
    uint8_t *head_flags = nullptr;
};
// What the text-keyed rounds key by (open_lists) and where the tied list stands
struct ListState {
    KeyParams Ptext;
    int s_sym = 0, tkb = 0;             // symbols per text round, bits of their packed key
    int64_t tiles = 0, depth = 0;       // RR_TILE-element tiles of the whole array; symbols the current order is sorted by (grows with the text rounds)
    bool ready = false;                 // (L.U, L.G, L.V) already hold the tied suffixes
};
enum class FirstRound { NONE, FINISHED32, FUSED64 };      // what ran straight from the sorted keys: fast_finish32, fused_first_text_round
// What rank_setup_and_text_rounds leaves for the doubling rounds.  sparse: few tied suffixes, ranks looked up without an ISA;
// isa_tail_ranks: the rank set-up of the dense route wrote tail ranks (k_rr_apply FTAIL)
struct RankSetup { bool sparse = false, isa_tail_ranks = false; };

// One device-resident build, phase by phase.  A phase takes what earlier phases decided or left (Route, InitialOrder, ListState, ...)
// and returns an SA_AMD_* status; build_device is the sequence.  The blocking 4-byte read-backs that steer the host (how many suffixes
// are still tied, how many groups, how many ranks changed) are the read_words calls inside the phases: each one names what it reads.
struct DeviceBuild : BuildCore {       // (BuildCore, host/refine_round.hpp: the inputs, the tied list L and the re-rank launchers)
    EarlyDownload *early = nullptr;     // host-pointer callers: the array starts travelling before the last rounds are done
    bool trace = false;
    double trace_t = 0;
    double lap() { const double t = now_ms(), d = t - trace_t; trace_t = t; return d; }
#ifdef SA_AMD_DIAG
    bool timing_only() const { return tn.timing_only_initial_sort; }      // diag library only: stop after the initial sort (array NOT finished)
#else
    bool timing_only() const { return false; }
#endif
    RoundState rs;                      // what one refinement round leaves for the next

    // Early download: called wherever (L.U, L.m) is the current tied list and every slot outside it is final
    int early_maybe_start()
    {
        if (!early || early->started || L.m <= 0 || L.m > early->threshold || !early->start) return SA_AMD_OK;
        if (!early->ev && hipEventCreateWithFlags(&early->ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return SA_AMD_OK; }
        hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, dSA, (uint32_t)n);   // reference src/saca.rs:13 (the first chunk carries it)
        LAUNCH_CHECK(st);
        HIP_TRY(hipMemsetAsync(w.early_bits, 0, (((size_t)n + 1 + 31) / 32 + EARLY_THREADS) * 4, st));
        if ((((uintptr_t)L.U) & 15) != 0) return SA_AMD_OK;       // (the list slabs are 256-byte aligned: cannot happen)
        PROF(KC_MISC, L.m, st, hipLaunchKernelGGL((k_early_mark), dim3(capped_grid(L.m, 256 * 8, 65536)), dim3(256), 0, st, (const uint32_t *)L.U, L.m, (uint32_t)early->off, w.early_bits));
        HIP_TRY(hipEventRecord(early->ev, st));
        early->started = true;
        early->m_snap = L.m;
        if (trace) fprintf(stderr, "suffix_array_amd: early download starts with %lld suffixes still tied\n", (long long)L.m);
        early->start(early->ev);
        return SA_AMD_OK;
    }
    // ... and when the array is complete: the final values of the marked entries among those the copy has taken
    int early_finish()
    {
        if (!early || !early->started) return SA_AMD_OK;
        early->covered = early->stop ? early->stop() : 0;
        if (early->covered > n + early->off) early->covered = n + early->off;
        early->holes = 0;
        if (early->covered <= 0) return SA_AMD_OK;
        const int64_t tiles_e = ceil_div(early->covered, EARLY_TILE);
        const int64_t words = ceil_div(early->covered, 32);
        // (bits beyond the covered entries inside the last word belong to entries that are downloaded later: harmless, they are
        // patched with their final values too when the host walks whole words -- the host stops at `covered`)
        PROF(KC_MISC, early->covered, st, hipLaunchKernelGGL((k_early_count), dim3((unsigned)tiles_e), dim3(EARLY_THREADS), 0, st,
                                                             (const uint32_t *)w.early_bits, words, w.early_cnt));
        PROF(KC_RR_SCAN, tiles_e, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.early_cnt, (uint32_t *)nullptr, tiles_e, w.early_cnt + tiles_e));
        uint32_t *holes = (uint32_t *)w.keysC;
        PROF(KC_MISC, early->covered, st, hipLaunchKernelGGL((k_early_gather), dim3((unsigned)tiles_e), dim3(EARLY_THREADS), 0, st,
                                                             (const uint32_t *)w.early_bits, words, (const uint32_t *)w.early_cnt,
                                                             (const uint32_t *)(dSA + 1 - early->off), holes));
        uint32_t total = 0;
        { const int rcw = read_words(&total, w.early_cnt + tiles_e, 4, st); if (rcw) return rcw; }
        early->holes = total;
        early->d_bits = w.early_bits; early->d_tile_off = w.early_cnt; early->d_holes = holes;
        return SA_AMD_OK;
    }

    // Bucket sort of the 32-bit first stage: which key bits do the global passes order?  16 (two passes of 8 bits) when an average
    // bucket fits the 10-pairs-per-thread shapes (n = 2^28: 4096 pairs; 2^29: 8192), 18 (two passes of NINE bits) for larger texts
    // (2^30: 2^18 buckets of 4096), 0 = four global passes.
    int choose_bucket_bits(const Route &R) const
    {
        if (tn.no_bucket_sort || n < tn.bucket_min_n || n <= 1) return 0;
        if (tn.bucket_bits == 18 && wide_ok()) return 18;
        if (tn.bucket_bits == 16) return 16;
        // (measured, random bytes and DNA: with the two key bits that travel in the values (key_source32) 18 bits win from about
        // 4.9e8 suffixes on -- 2^29: 9.09 against 9.36 ms --, without them only where 16 bits no longer fit).  Asked before the probe
        // has set top_shift, so for the 32 that whole keys give: under SA_AMD_KEY_BITS < 64 the stage shifts by less and builds a
        // key array, and the 18 bits chosen here for value bits get none -- that case is kept as it was.  (== 2: 30-bit indices; n >= 64 here.)
        const bool value_bits = (n >> 16) > 7500 && key_source32(R, 18, 32).val_extra == 2;
        if (value_bits && (n >> 18) * 10 <= bucket_cap_max() * 9) return 18;
        if ((n >> 16) * 10 <= bucket_cap(2) * 9) return 16;
        if (wide_ok() && (n >> 18) * 10 <= bucket_cap_max() * 9) return 18;
        if ((n >> 16) * 10 <= bucket_cap_max() * 9) return 16;
        return 0;
    }
    bool wide_ok() const { return onesweep_on(w.ss, tn) && tn.onesweep32_shape == 0; }      // nine-bit digits, keys read from the text: single-pass engine, default tile
    // Where the 32-bit stage's first global pass over `top_bits` (0: four passes) takes its keys, the stage shifting by top_shift.
    // A text of all 256 byte values (code = byte, 8 symbols per key): the top 32 key bits are four text bytes -- the pass reads
    // them from the text (a quarter of the bytes) and no key array is built in front of it; with four symbols (DNA) the bit-packed
    // text is the stream of keys: it is packed first (n / 4 bytes instead of a key array of 4n), counted and read as it stands.
    // Key bits for free: an index below 2^g_bits leaves 32 - g_bits bits of the value word unused, and the bucket sort stages
    // 16 bits per pair of which 32 - top_bits are low key bits.  When both have room (texts of 0.6 - 1 GiB: 18 top bits, 30-bit
    // indices) the first pass puts the two key bits BEHIND the 32 there and the bucket sort orders 34 bits: a quarter of the ties
    // on all 32 bits are left for its round on the low key bits (1 GiB of DNA: 22 % of the suffixes -> 6 %).
    struct KeySource32 { bool text_keys = false, packed_keys = false; int val_extra = 0; };      // (neither: a key array; val_extra: low key bits that travel in the values)
    KeySource32 key_source32(const Route &R, int top_bits, int top_shift) const
    {
        KeySource32 s;
        // (iota: the values are the indices and the first pass is counted)
        const bool text_route = top_bits != 0 && iota(R) && top_shift == 32 && wide_ok() && !tn.no_text_keys;
        s.text_keys = text_route && R.sigma == 256 && R.P.bits == 8;      // (eight bits a symbol: never packed)
        s.packed_keys = text_route && R.sigma == 4 && R.P.bits == 2 && packs_text(R.P);
        if ((s.text_keys || s.packed_keys) && !tn.no_value_bits) {
            s.val_extra = std::max(0, std::min(std::min(32 - g_bits, BK_MAX_LBITS - (32 - top_bits)), 2));
        }
        return s;
    }
    // alphabets of 2, 4 or 16 symbols: k_build_keys also writes the text as bit-packed codes, which every later random
    // read of the text uses instead (a key becomes a bit field of two words; DNA shrinks to a quarter: cache-resident)
    bool packs_text(const KeyParams &P) const { return (P.bits == 1 || P.bits == 2 || P.bits == 4) && n >= 64 && !tn.no_packed_text; }
    uint8_t *packed_out(const Route &R) const { return R.Pp.packed ? w.packed : (uint8_t *)nullptr; }      // where the key building writes it
    bool flat_rule_applies() const { return n >= 2 && n < tn.top32_probe_min_n && n < ((int64_t)1 << 24) && !tn.no_flat_rule; }

    // the rank set-up of the dense route (ISA_MODE 0: direct ISA stores, 2: ranks for the binned scatter): tail or head ranks,
    // groups from the flags or from the sorted keys
    template <int ISA_MODE>
    int rr_apply_setup(const InitialOrder &O, bool tail, RrApply a)
    {
        const uint64_t *k = O.sr.keys;
        a.status = O.head_flags;
        if (O.head_flags)
            return tail ? rr_apply<true, false, ISA_MODE, uint64_t, true, true>(k, a) : rr_apply<true, false, ISA_MODE, uint64_t, false, true>(k, a);
        return tail ? rr_apply<true, false, ISA_MODE, uint64_t, true>(k, a) : rr_apply<true, false, ISA_MODE>(k, a);
    }
    // Flags were emitted but the route that follows reads the sorted keys (compaction for the text rounds, rank look-ups of the
    // sparse rounds): sr.keys[i] = the initial key of suffix SA[i], by the device function those look-ups compare with.  Rare in
    // real use (the flags are asked for only when the dense route is expected) and dear: about 50 ms at 256 MiB with gram keys.
    int rebuild_sorted_keys(const Route &R, InitialOrder &O)
    {
        if (!O.head_flags) return SA_AMD_OK;
        PROF(KC_GATHER, n, st, hipLaunchKernelGGL((k_keys_of_suffixes), dim3(capped_grid(n, GK_THREADS, 65536)), dim3(GK_THREADS), 0, st, dT, R.Pp, n, (const uint32_t *)SA, O.sr.keys));
        O.head_flags = nullptr;
        if (trace) fprintf(stderr, "suffix_array_amd: sorted keys rebuilt from the suffix array (the route taken reads them)\n");
        return SA_AMD_OK;
    }
    // what every re-rank straight from the initial order shares: all n slots in, the first tied list out
    RrApply first_args(uint32_t n_text, uint32_t *has_isa = nullptr) const      // (n_text = 0 with has_isa: compaction only)
    {
        RrApply a;
        a.V = SA; a.m = n; a.SA = SA; a.ISA = w.isa; a.Uo = L.U; a.Go = L.G; a.Vo = L.V; a.n_text = n_text; a.has_isa = has_isa;
        return a;
    }
    // ---- launches that several phases share ----
    // Duplicates among the S sampled keys in w.keysA -> w.total[0] (the caller reads it back): counted in a hash table (4 entries
    // per sample, in the other key buffer) instead of sorting the sample.  zero_bytes: the words of w.total the caller will read.
    int count_sample_dups(int64_t S, size_t zero_bytes)
    {
        const uint32_t H = (uint32_t)S * 4u;
        HIP_TRY(hipMemsetAsync(w.keysB, 0xff, (size_t)H * 8, st));
        HIP_TRY(hipMemsetAsync(w.total, 0, zero_bytes, st));
        PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_count_sample_dups), dim3(capped_grid(S, 256, 4096)), dim3(256), 0, st, (const uint64_t *)w.keysA, S,
                                                (unsigned long long *)w.keysB, H - 1u, w.total));
        return SA_AMD_OK;
    }
    // the 64-bit initial keys (plain or gram form) into w.keysA, with the first sort pass's digit counts when the sort wants them
    int build_keys64(const Route &R, const FirstCounts &fc, bool counted)
    {
        const int nb0 = R.key_bits < RADIX_BITS ? R.key_bits : RADIX_BITS;
        uint32_t *vals0 = iota(R) ? (uint32_t *)nullptr : w.valsA;
        PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((R.P.gram > 0 ? k_build_keys<false, true> : k_build_keys<false>), dim3((unsigned)ceil_div(ceil_div(n, KB_TILE), KB_TPW)),
                                                      dim3(KB_THREADS), 0, st, dT, n, R.P, w.keysA, vals0,
                                                      (uint32_t *)nullptr, 0, packed_out(R), counted ? fc.counts : (uint32_t *)nullptr, fc.chunk_elems, fc.G, (1u << nb0) - 1u, 0));
        return SA_AMD_OK;
    }
    // the records of the fast finish of the 32-bit first stage (k_finish_sorted, or k_bucket_sort on its behalf) start from zero
    int zero_finish_records()
    {
        HIP_TRY(hipMemsetAsync(w.surv_bits, 0, ((size_t)n + 31) / 32 * 4, st));
        HIP_TRY(hipMemsetAsync(w.tcnt, 0, (size_t)ceil_div(n, RR_TILE) * 4, st));
        HIP_TRY(hipMemsetAsync(w.thead, 0, (size_t)ceil_div(n, RR_TILE) * 4, st));
        HIP_TRY(hipMemsetAsync(w.total, 0, 16, st));
        HIP_TRY(hipMemsetAsync(w.chg, 0, (size_t)RR_CHG_COUNTERS * 32 * 4, st));
        return SA_AMD_OK;
    }

    // 1-2. which byte values occur -> symbol codes and key geometry; entropy probe, repeat probe, gram keys (read-backs: the 256 presence flags, two duplicate counts, the number of grams in use)
    int geometry_and_probes(Route &R)
    {
        int rc;
        // 1. sigma = 256 histogram -> symbol codes, bits per symbol, symbols per key
        HIP_TRY(hipMemsetAsync(w.hist, 0, 256 * 4, st));
        // (texts below the entropy probe's size: with counts, for the flat-histogram rule below)
        if (flat_rule_applies()) PROF(KC_BYTE_HIST, n, st, hipLaunchKernelGGL((k_byte_hist_counts), dim3(capped_grid(ceil_div(n, 16), BH_THREADS, 256)), dim3(BH_THREADS), 0, st, dT, n, w.hist));
        else PROF(KC_BYTE_HIST, n, st, hipLaunchKernelGGL((k_byte_hist), dim3(capped_grid(ceil_div(n, 16), BH_THREADS, 2048)), dim3(BH_THREADS), 0, st, dT, n, w.hist));
        uint32_t hist[256];
        { const int rcw = read_words(hist, w.hist, sizeof(hist), st); if (rcw) return rcw; }
        // Texts too short for the entropy probe (a sampling pass and a read-back of its own): byte values that are all equally
        // frequent (order-0 entropy = log2 of their number: random bytes, random DNA) say "no structure at order 0", and then
        // log2 n + 20 key bits separate nearly every suffix -- five radix passes instead of eight at 1 MiB (random bytes 0.36 ->
        // 0.25 ms; English-like text, whose histogram is anything but flat, would pay 0.50 -> 0.71 for the same keys and keeps all
        // 64 bits).  A flat text that does repeat (a period, a block copied twice) is ordered by the rounds as before.
        int kb_max = tn.key_bits_max;
        if (flat_rule_applies()) {
            double h0 = 0.0; int used = 0;
            for (int c = 0; c < 256; ++c)
                if (hist[c]) { const double pc = (double)hist[c] / (double)n; h0 -= pc * std::log2(pc); ++used; }
            if (used >= 2 && h0 > std::log2((double)used) - 0.01) {
                int kb = (bit_length((uint64_t)(n - 1)) + 20 + 7) / 8 * 8;
                if (kb < 32) kb = 32;
                if (kb < kb_max) kb_max = kb;
                R.flat_text = true;
            }
        }
        KeyParams &P = R.P;
        int &key_bits = R.key_bits, &top_shift = R.top_shift;
        key_bits = make_key_params(hist, &P, &R.sigma, kb_max);      // (gram keys, step 2c, may shorten it)
        local.sigma = R.sigma; local.bits_per_symbol = P.bits; local.symbols_per_key = P.k;
        if (R.sigma == 1 && !tn.no_unary_shortcut) {
            // one byte value repeated: every suffix is a proper prefix of every longer one, the order is by length.  (The general
            // path gets there too -- 23 doubling rounds over one group of n members, 214 ms at 256 MiB -- and stays tested.)
            PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_fill_descending), dim3(capped_grid(n, 256 * 16, 16384)), dim3(256), 0, st, SA, n));
            R.unary = true;
            return SA_AMD_OK;
        }

        g_bits = bit_length((uint64_t)(n - 1 > 0 ? n - 1 : 1));
        R.bucket_top_bits = choose_bucket_bits(R);
        R.force_dense = tn.force_dense;
        R.text_ok = !R.force_dense && !tn.no_text_rounds;
        rs.local_ok = !tn.no_local_sort;

        // 2. entropy probe: do the top 32 key bits already separate (almost) all suffixes?  Then the initial
        //    sort only needs those 4 digits and a cheap round on the low bits finishes the few ties.
        if (R.text_ok && rs.local_ok && key_bits > 32 && !tn.no_top32) {
            bool use = tn.force_top32;
            if (!use && n >= tn.top32_probe_min_n) {
                // 2^20 samples, fewer for texts below 8 Mi suffixes (a power of two: the duplicate count hashes into 4 S slots)
                int64_t S = (int64_t)1 << 20;
                while (S > 1024 && S * 8 > n) S >>= 1;
                PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_sample_keys), dim3((unsigned)ceil_div(S, GK_THREADS)), dim3(GK_THREADS), 0, st, dT, P, n, S,
                                                        key_bits - 32, w.keysA));
                if ((rc = count_sample_dups(S, 8))) return rc;
                // the same samples, counted per bucket of the bucket sort: an estimate of its largest bucket (word 1 of the read-back)
                const int tb = R.bucket_top_bits;
                if (tb) {
                    HIP_TRY(hipMemsetAsync(w.keysC, 0, ((size_t)1 << tb) * 4, st));
                    // (a quarter of the samples is enough to tell a bucket with a tenth of the text from a flat one, and a quarter of the atomics)
                    PROF(KC_MISC, S / 4, st, hipLaunchKernelGGL((k_sample_bucket_hist), dim3((unsigned)ceil_div(S / 4, BK_STARTS_THREADS)), dim3(BK_STARTS_THREADS), 0, st,
                                                            (const uint64_t *)w.keysA, S / 4, tb, (uint32_t *)w.keysC));
                    PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_u32_max), dim3((unsigned)(((size_t)1 << tb) / BK_STARTS_THREADS)), dim3(BK_STARTS_THREADS), 0, st,
                                                            (const uint32_t *)w.keysC, 1u << tb, w.total + 1));
                }
                uint32_t dups = 0;
                {
                    uint32_t two[2] = { 0, 0 };
                    const int rcw = read_words(two, w.total, 8, st); if (rcw) return rcw;
                    dups = two[0];
                    // (a flat text of 2^28 bytes: 4 samples per bucket on average, the fullest holds about 14 -> 14 336 estimated, 4400 true)
                    const double est = (double)two[1] * (double)n / (double)(S / 4);
                    if (tb && est > 3.0 * (double)bucket_cap_max()) {
                        R.bucket_top_bits = 0;
                        if (trace) fprintf(stderr, "suffix_array_amd: bucket sort of the 32-bit first stage: largest bucket estimated at %.0f suffixes -> four global passes\n", est);
                    }
                }
                // c - 1 per value seen c times under-counts pairs only when values repeat often, which is the
                // "do not" case anyway; expected number of other suffixes sharing the top bits with a given one:
                const double p32 = (double)n * 2.0 * (double)dups / ((double)S * (double)S);
                use = p32 < (double)tn.top32_partners_x100 / 100.0;
                double p64 = -1.0;
                if (!use && p32 < 4.0 * (double)tn.top32_collisions_x100 / 100.0) {
                    // Not "almost all separated" -- but WHY do suffixes share their top 32 bits?  Chance collisions (a small or
                    // skewed alphabet: few partners each, told apart by the low key bits in one pass over the sorted keys) or
                    // repeats (they share the low bits too and go to the refinement rounds either way).  The same sample,
                    // whole keys: the partners a suffix has on all key bits.  Measured (tools/top32_threshold.py, 1 GiB): sigma 16
                    // skewed, 2.5 partners on 32 bits and none on 64: 42 ms against 74 ms with full keys; DNA with 20 % in
                    // repeats (0.72 / 0.35): 118 against 137 ms; 40 % in repeats (0.82 / 0.45): 154 against 143 ms -- hence 0.8 x the threshold for those.
                    PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_sample_keys), dim3((unsigned)ceil_div(S, GK_THREADS)), dim3(GK_THREADS), 0, st, dT, P, n, S,
                                                            -1, w.keysA));
                    if ((rc = count_sample_dups(S, 4))) return rc;
                    uint32_t dups64 = 0;
                    { const int rcw = read_words(&dups64, w.total, 4, st); if (rcw) return rcw; }
                    const double chance = (double)S * (double)S / 8589934592.0;           // 32-bit hash collisions among S samples
                    const double d64 = (double)dups64 > chance ? (double)dups64 - chance : 0.0;
                    p64 = (double)n * 2.0 * d64 / ((double)S * (double)S);
                    use = p64 < 0.8 * (double)tn.top32_partners_x100 / 100.0 && p32 - p64 < (double)tn.top32_collisions_x100 / 100.0;
                }
                if (trace) fprintf(stderr, "suffix_array_amd: entropy probe: %u duplicates of the top 32 key bits among %lld samples -> %.3f expected partners per suffix "
                                           "(on all key bits: %.3f) -> %s\n", dups, (long long)S, p32, p64, use ? "32-bit first stage" : "full keys");
            }
            if (use) top_shift = key_bits - 32;
        }
        local.top32_first = top_shift ? 1 : 0;
        // 2b. repeat probe (texts the first probe did not send to the 32-bit route): the fraction of suffixes that share
        //     2k symbols with another suffix.  Many (copied passages, a corpus): the text-keyed rounds cannot finish, so rank
        //     doubling starts right after the initial sort (measured on C3: 64 ms against 68 ms); few: text-keyed rounds.
        if (R.text_ok && rs.local_ok && !top_shift && !tn.no_repeat_probe && n >= ((int64_t)1 << 24)) {      // (text_ok: not force_dense)
            const int64_t S = (int64_t)1 << 20;
            PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_sample_repeat_keys), dim3((unsigned)ceil_div(S, GK_THREADS)), dim3(GK_THREADS), 0, st, dT, P, n, S,
                                                    w.keysA));
            if ((rc = count_sample_dups(S, 4))) return rc;
            uint32_t dups = 0;
            { const int rcw = read_words(&dups, w.total, 4, st); if (rcw) return rcw; }
            const double chance = (double)S * (double)S / 8589934592.0;           // 32-bit hash collisions among S samples
            const double frac = ((double)dups - chance) * (double)n / ((double)S * (double)S);
            R.probe_dense = frac > 0.04;
            if (trace) fprintf(stderr, "suffix_array_amd: repeat probe: %u duplicates among %lld samples (repeat index %.3f, threshold 0.04) -> %s\n",
                               dups, (long long)S, frac, R.probe_dense ? "rank doubling from the start" : "text-keyed rounds");
        }

        // 2c. gram keys (texts that did not take the 32-bit route): choose_gram_keys measures and decides; the probes above keep
        //     using the plain key
        if (!top_shift && !tn.no_gram_keys && n >= tn.gram_min_n && n >= 2 && R.sigma >= 2 && tn.key_bits_max == 64) {
            if ((rc = choose_gram_keys(dT, n, &P, &key_bits, w, st, tn, trace))) return rc;
            local.bits_per_symbol = P.bits; local.symbols_per_key = P.k;
        }
        R.Pp = P;
        if (packs_text(P)) R.Pp.packed = w.packed;
        return SA_AMD_OK;
    }

    // 4b. the 32-bit first stage: the top 32 key bits as (u32, u32) pairs -- two global passes + the in-LDS bucket sort, or four
    //     global passes (read-back: the largest bucket).  Its keys for passes over `top_bits` (key_source32) and the sort they go into:
    bool iota(const Route &R) const { return n >= 2 && R.key_bits > 0; }      // value of pair i = i: not stored by k_build_keys, the first sort pass takes the index (saves 8 B / suffix)
    int top32_keys(const Route &R, int top_bits, SortJob<uint32_t> *job)
    {
        // the first radix pass's digit histogram comes out of k_build_keys (keys in registers there): one read of every key less
        const FirstCounts fc = sort_first_counts(w.ss, tn, n, true);
        const bool counted = n > 1;
        const int rbits = top_bits == 18 ? 9 : RADIX_BITS;
        const KeySource32 ks = key_source32(R, top_bits, R.top_shift);
        uint8_t *const packed_out = this->packed_out(R);
        if (counted) HIP_TRY(hipMemsetAsync(fc.zero_ptr, 0, fc.zero_bytes, st));
        if (ks.text_keys || ks.packed_keys) {
            int split = 2048 / fc.G;
            while (split > 1 && fc.chunk_elems / split < 16384) split /= 2;
            const int64_t sub = (ceil_div(fc.chunk_elems, split) + 15) & ~(int64_t)15;
            if (ks.packed_keys) {
                PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_pack_text2), dim3(capped_grid(ceil_div(n, 16), 256, 16384)), dim3(256), 0, st, dT, n, R.P, packed_out));
                PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_packed2_upsweep32), dim3((unsigned)(fc.G * split)), dim3(SORT_THREADS), 0, st, (const uint8_t *)packed_out, n,
                                                              fc.counts, 32 - top_bits, (1u << rbits) - 1u, fc.chunk_elems, fc.G, split, sub));
            } else
            PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_text_upsweep32), dim3((unsigned)(fc.G * split)), dim3(SORT_THREADS), 0, st, dT, n, fc.counts,
                                                          32 - top_bits, (1u << rbits) - 1u, fc.chunk_elems, fc.G, split, sub));
        } else
        PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_build_keys<true>), dim3((unsigned)ceil_div(ceil_div(n, KB_TILE), KB_TPW)), dim3(KB_THREADS), 0, st, dT, n, R.P,
                                                      (uint64_t *)nullptr, iota(R) ? (uint32_t *)nullptr : w.valsA, (uint32_t *)w.keysA, R.top_shift, packed_out,
                                                      counted ? fc.counts : (uint32_t *)nullptr, fc.chunk_elems, fc.G, (1u << rbits) - 1u, top_bits ? 32 - top_bits : 0));
        *job = SortJob<uint32_t>{ (uint32_t *)w.keysA, w.valsA, (uint32_t *)w.keysB, w.valsB, n, top_bits ? 32 - top_bits : 0, 32 };
        job->iota = iota(R); job->first_counted = counted;
        if (top_bits) {
            job->rbits = rbits;
            job->text = ks.text_keys ? dT : (ks.packed_keys ? (const uint8_t *)packed_out : (const uint8_t *)nullptr);
            job->text_n = n; job->text_bits = ks.packed_keys ? 2 : 8;
            job->val_extra = ks.val_extra;
        }
        return SA_AMD_OK;
    }
    // Bucket route: two global passes over the top 16 key bits + one pass that orders every bucket (= value of those bits) in LDS,
    // when an average bucket fits a workgroup well (n = 2^28: 4096 pairs, 2^29: 8192); larger texts take two passes of NINE bits
    // (2^30: 2^18 buckets of 4096).  May decline (*done = false, nothing written to SA): a text whose LARGEST bucket fits no
    // workgroup -- known only once the two passes have run -- builds its keys again and takes the four global passes.
    int top32_bucket_route(const Route &R, InitialOrder &O, bool *done)
    {
        int rc;
        const int top_bits = R.bucket_top_bits;
        SortJob<uint32_t> job{}; SortResult<uint32_t> s32;
        if ((rc = top32_keys(R, top_bits, &job)) || (rc = sort_pairs32(job, w.ss, st, tn, &s32, &local))) return rc;
        uint32_t *kout = (s32.keys == job.keys_in) ? job.keys_alt : job.keys_in;
        bool fused = false; uint32_t largest = 0;
        // the round on the low key bits of the suffixes tied on all 32 (fast_finish32) in the same launch
        const bool fuse = rs.local_ok && !tn.no_fused_finish && !tn.no_bucket_finish && !timing_only();
        BucketFinish F = BucketFinish(); KeySrc K = KeySrc();
        if (fuse) {
            if ((rc = zero_finish_records())) return rc;
            F.T = dT; F.n = n; F.cap = tn.group_cap; F.surv_bits = w.surv_bits; F.surv_head = w.isa; F.tile_cnt = w.tcnt; F.counters = w.total;
            K.mode = KS_LOWKEY; K.kb = R.top_shift;
        }
        // (Pp: the text is packed by now, the fused round's text look-ups take the bit-packed text, a quarter of the lines)
        if ((rc = bucket_sort32(s32.keys, s32.vals, kout, SA, n, top_bits, w.bk_start, w.ss.err + 2, st, tn, done, &largest,
                                fuse ? &F : nullptr, &R.Pp, &K, &fused, job.val_extra))) return rc;
        O.bucket_finished = *done && fused;
        if (trace) fprintf(stderr, "suffix_array_amd: 32-bit first stage: %d global passes over the top %d key bits, largest bucket %u -> %s\n", s32.passes, top_bits, largest,
                           *done ? (fused ? "low bits and ties on all 32 ordered bucket by bucket in LDS" : "low bits ordered bucket by bucket in LDS")
                                 : "too large: keys rebuilt, four global passes");
        if (!*done) return SA_AMD_OK;      // (nothing was launched: the finish buffers are zeroed again by whoever uses them)
        local.sort_passes += 1; local.sorted_elements += n;
        O.sorted32 = kout;
        O.sr.vals = SA; O.sr.passes = s32.passes + 1;
        O.sr.keys = (kout == job.keys_in) ? w.keysA : w.keysB;
        return SA_AMD_OK;
    }
    // ... or four global passes over a key array, the last one writing into SA
    int top32_four_passes(const Route &R, InitialOrder &O)
    {
        int rc;
        SortJob<uint32_t> job{}; SortResult<uint32_t> s32;
        if ((rc = top32_keys(R, 0, &job))) return rc;
        job.final_vals = SA;
        if ((rc = sort_pairs32(job, w.ss, st, tn, &s32, &local))) return rc;
        O.sorted32 = s32.keys;
        O.sr.vals = s32.vals; O.sr.passes = s32.passes;
        O.sr.keys = (s32.keys == job.keys_in) ? w.keysA : w.keysB;      // the 8n-byte buffer that now holds the sorted 32-bit keys
        return SA_AMD_OK;
    }

    // 3-4. packed keys and the initial LSD sort, the last pass writing straight into SA
    int initial_sort(const Route &R, InitialOrder &O)
    {
        int rc;
        // 3. packed keys, 4. initial sort: all key bits as (u64 key, u32 suffix) pairs, or only the top 32 bits as
        //    (u32, u32) pairs in 12 Ki-element tiles -- two thirds of the bytes per pass and half the passes
        SortResult<uint64_t> &sr = O.sr;
        sr.keys = w.keysA; sr.vals = w.valsA; sr.passes = 0;
        if (R.Pp.packed) HIP_TRY(hipMemsetAsync(w.packed + (size_t)(n >> 3) * R.P.bits, 0, 64, st));     // the padding behind the last whole group
        if (R.top_shift) {
            bool done = false;
            if (R.bucket_top_bits && (rc = top32_bucket_route(R, O, &done))) return rc;
            if (!done && (rc = top32_four_passes(R, O))) return rc;
        } else {
            const FirstCounts fc = sort_first_counts(w.ss, tn, n, false);
            const bool counted = n > 1 && R.key_bits > 0;
            if (counted) HIP_TRY(hipMemsetAsync(fc.zero_ptr, 0, fc.zero_bytes, st));
            if ((rc = build_keys64(R, fc, counted))) return rc;
            // (a text of ONE byte value -- a zero-filled file -- has the same key everywhere but at its end: its passes are the identity
            // and are looked for; any other text does not pay the read-backs)
            // diagnostic library, SA_AMD_SAMPLE_SORT=1 (a measured dead end, profiles/r04_sample_sort_64.txt): the sample sort -- two
            // distribution passes over quantile digits + every bucket ordered in LDS -- instead of one LSD pass per digit
            bool ss_done = false;
#ifdef SA_AMD_DIAG
            if (iota(R) && counted && tn.sample_sort && n >= tn.sample_sort_min_n && R.key_bits > 32 && onesweep_on(w.ss, tn) && !timing_only()) {
                const size_t need_big = ((size_t)ceil_div(n, SS_TILE) + SS_WAYS) * SS_IDS2 * 4;
                if (need_big <= (size_t)n * 4 && (size_t)n * 4 >= ((size_t)4 << 20)) {
                    rc = sample_sort64(w.keysA, w.keysB, w.keysC, w.valsA, w.valsB, w.U0, w.U1, w.isa, w.G0, w.bk_start, SA, n, R.key_bits, w.ss, st, &local, tn,
                                       &ss_done, trace);
                    if (rc) return rc;
                    if (ss_done) { sr.keys = w.keysB; sr.vals = SA; sr.passes = 3; sr.skipped = 0; }
                    else {
                        // (cannot sort this text in workgroup-sized buckets: the keys again, then the LSD engine)
                        HIP_TRY(hipMemsetAsync(fc.zero_ptr, 0, fc.zero_bytes, st));
                        if ((rc = build_keys64(R, fc, true))) return rc;
                    }
                }
            }
#endif
            if (!ss_done) {
            // Group-start flags instead of sorted keys from the last pass (head_flags above): asked for when the dense route is
            // expected -- its first re-rank is the only reader of the sorted keys then.  Tuning::head_flags 0: never, 2: always
            // (the routes that need the keys rebuild them: rebuild_sorted_keys); diagnostic library only.
            const bool want_flags = tn.head_flags != 0 && (tn.head_flags == 2 || R.dense_expected()) && flags_slab_ok && onesweep_on(w.ss, tn) && !timing_only() &&
                                    !tn.fused64 && n >= 2 && R.key_bits > 0;
            SortJob<uint64_t> job{ w.keysA, w.valsA, w.keysB, w.valsB, n, 0, R.key_bits };
            job.final_vals = SA;
            job.iota = iota(R); job.may_skip = R.sigma == 1; job.first_counted = counted;
            job.head_flags = want_flags ? (uint8_t *)w.keysC : (uint8_t *)nullptr;
            if ((rc = sort_pairs(job, w.ss, st, tn, &sr, &local))) return rc;
            if (want_flags && sr.passes > 0 && sr.vals == SA) O.head_flags = (uint8_t *)w.keysC;      // (the last pass always runs: it delivers into SA)
            if (trace && O.head_flags) fprintf(stderr, "suffix_array_amd: initial sort: the last pass wrote group-start flags, not the sorted keys\n");
            }
        }
        if (sr.vals != SA)     // n == 1: no pass ran, the values are still in the input buffer
            PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_copy_u32), dim3(1), dim3(256), 0, st, sr.vals, SA, n));
        return SA_AMD_OK;
    }

    // 4. the tied list's buffers and what the text-keyed rounds key by
    void open_lists(const Route &R, ListState &T)
    {
        const KeyParams &P = R.Pp;
        L.U = w.U0; L.Un = w.U1; L.G = w.G0; L.Gn = w.G1;
        L.V = w.valsA; L.m = 0;
        L.rkA = w.keysA; L.rkB = w.keysB;          // key buffers of the refinement rounds
        T.tiles = ceil_div(n, RR_TILE); T.depth = P.k;
        // Text-keyed rounds pack their symbols as bit fields of ceil(log2 sigma) bits whatever the alphabet: a secondary key only
        // has to preserve the order inside one round, and the base-sigma form costs a 64-bit multiply per symbol in kernels
        // that are instruction-bound (k_group_sort: 26 ps per suffix however small the text).  English-like sigma = 56: six
        // symbols in 36 bits either way.
        T.Ptext = P;
        if (P.bits == 0) T.Ptext.bits = bit_length(P.sigma - 1);
        T.Ptext.gram = 0;                                    // (gram ranks are the initial keys' business only)
        T.s_sym = (64 - g_bits) / T.Ptext.bits;              // (64 - g_bits: bits left below the group head)
        if (T.s_sym > 64) T.s_sym = 64;
        T.tkb = T.s_sym * T.Ptext.bits;
    }

    // fast finish of the 32-bit first stage: one pass orders every small group by its low key bits in place (k_finish_sorted);
    // only if some group is too large for it do group_heads and finish_top32_ties run instead (read-back: tied counts)
    int fast_finish32(const Route &R, const InitialOrder &O, ListState &T, FirstRound *first)
    {
        int rc;
        if (!(R.top_shift && rs.local_ok && !tn.no_fused_finish && !timing_only())) return SA_AMD_OK;
        const int64_t tiles = T.tiles;
        uint32_t *surv_bits = w.surv_bits, *surv_head = w.isa;  // (the ISA is not in use before the doubling rounds)
        if (!O.bucket_finished) {      // (else k_bucket_sort has done this round while it had the buckets in LDS, into the same records)
            if ((rc = zero_finish_records())) return rc;
            KeySrc K = KeySrc(); K.mode = KS_LOWKEY; K.kb = R.top_shift;
            PROF(KC_FINISH, n, st, hipLaunchKernelGGL((k_finish_sorted<uint32_t, KS_LOWKEY, false>), dim3((unsigned)ceil_div(n, FT_TILE)), dim3(FT_THREADS),
                                                     0, st, O.sorted32, SA, dT, R.Pp, n, K, tn.group_cap, surv_bits, surv_head, w.tcnt, w.total, (uint32_t *)nullptr,
                                                     (uint32_t *)nullptr, (uint32_t *)nullptr));
            // (k_bucket_sort counts its survivors itself: the scan of the tiles' counts runs only if there are any)
            PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total));
        }
        uint32_t words[ROUND_WORDS];         // (the tied-slot counts are spread over w.chg, directly behind w.total)
        { const int rcw = read_words(words, w.total, sizeof(words), st); if (rcw) return rcw; }
        // still tied on 64 bits (k_bucket_sort counts them in w.chg), members of groups nobody owned, tied on 32 bits
        const uint32_t tied64 = O.bucket_finished ? (uint32_t)chg_sum(words, 1) : words[0], unowned = words[1], tied32 = (uint32_t)chg_sum(words);
        if (O.bucket_finished && tied64 != 0 && unowned == 0)
            PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total));
        if (unowned != 0) return SA_AMD_OK;
        *first = FirstRound::FINISHED32;
        L.m = tied64;
        local.locally_sorted += tied32; local.unresolved_after_initial = L.m;
        if (L.m > 0) {
            PROF(KC_RR_APPLY, n, st, hipLaunchKernelGGL((k_surv_compact), dim3((unsigned)tiles), dim3(256), 0, st, (const uint32_t *)surv_bits,
                                                        (const uint32_t *)surv_head, (const uint32_t *)SA, n, (const uint32_t *)w.tcnt,
                                                        (const uint32_t *)w.total, L.U, L.G, L.V));
            L.keys_beside(w, O.sr.keys);
            T.ready = true;
        }
        return SA_AMD_OK;
    }

    // Opt-in (SA_AMD_FUSED64=1): measured on C3 the one-pass round costs 8.2 ms against the 4.3 ms of k_group_sort on the tied
    // list -- with 68 % of the slots tied the work list is six entries per thread -- and the whole build 31.0 instead of 28.8 ms.
    // (SA_AMD_SPARSE_DIV moves the text-round / doubling boundary for the tests: then the general route decides, as before)
    int fused_first_text_round(const Route &R, const InitialOrder &O, ListState &T, FirstRound *first)
    {
        int rc;
        if (R.top_shift || !R.text_ok || !rs.local_ok || T.s_sym <= 0 || !tn.fused64 || tn.no_fused_finish || tn.sparse_div_set || timing_only()) return SA_AMD_OK;
        const int64_t tiles = T.tiles;
        // the first text-keyed round straight from the sorted keys (k_finish_sorted): groups of up to `cap` members are
        // ordered in place by the next s_sym symbols, their still-tied members recorded by slot; the members of larger
        // groups are listed (k_todo_compact) and take the general route (RefineRound::run<NO_RERANK> + re-rank), joining the same record;
        // k_surv_compact then lists everything that is still tied, in slot order, for the second round
        const int cap = tn.group_cap;
        const int64_t ft_tiles = ceil_div(n, FT_TILE);
        uint32_t *surv_head = w.isa;
        HIP_TRY(hipMemsetAsync(w.surv_bits, 0, ((size_t)n + 31) / 32 * 4, st));
        HIP_TRY(hipMemsetAsync(w.todo_bits, 0, ((size_t)n + 31) / 32 * 4, st));
        HIP_TRY(hipMemsetAsync(w.ft_cnt, 0, (size_t)(ft_tiles + 1) * 4, st));
        HIP_TRY(hipMemsetAsync(w.ft_head, 0, (size_t)(ft_tiles + 1) * 4, st));
        HIP_TRY(hipMemsetAsync(w.surv_cnt, 0, (size_t)tiles * 4, st));
        HIP_TRY(hipMemsetAsync(w.thead, 0, (size_t)tiles * 4, st));
        HIP_TRY(hipMemsetAsync(w.total, 0, 32, st));
        HIP_TRY(hipMemsetAsync(w.chg, 0, (size_t)RR_CHG_COUNTERS * 32 * 4, st));
        KeySrc K = KeySrc(); K.mode = KS_TEXT; K.h = T.depth; K.s = T.s_sym; K.kb = T.tkb;
        PROF(KC_FINISH, n, st, hipLaunchKernelGGL((k_finish_sorted<uint64_t, KS_TEXT, true>), dim3((unsigned)ft_tiles), dim3(FT_THREADS), 0, st,
                                                 (const uint64_t *)O.sr.keys, SA, dT, T.Ptext, n, K, cap, w.surv_bits, surv_head, w.surv_cnt, w.total,
                                                 w.todo_bits, w.ft_cnt, w.ft_head));
        PROF(KC_RR_SCAN, ft_tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.ft_cnt, w.ft_head, ft_tiles, w.total + 3));
        uint32_t words[ROUND_WORDS];
        { const int rcw = read_words(words, w.total, sizeof(words), st); if (rcw) return rcw; }
        const int64_t tied0 = (uint32_t)chg_sum(words), m_todo = words[3];      // tied after the initial sort, members left to the general route
        local.unresolved_after_initial = tied0;
        local.locally_sorted += tied0 - m_todo;
        L.keys_beside(w, O.sr.keys);
        if (m_todo > 0) {
            PROF(KC_RR_APPLY, n, st, hipLaunchKernelGGL((k_todo_compact<uint64_t>), dim3((unsigned)ft_tiles), dim3(FT_THREADS), 0, st,
                                                        (const uint64_t *)O.sr.keys, (const uint32_t *)SA, n, (const uint32_t *)w.todo_bits,
                                                        (const uint32_t *)w.ft_cnt, (const uint32_t *)w.ft_head, (const uint32_t *)(w.total + 3),
                                                        L.U, L.G, L.V));
            L.m = m_todo;
            RoundState own;                                    // (a switch of its own: large groups, the global sort does the work either way)
            own.local_ok = true;
            RefineRound round(*this, T.Ptext, K, own);
            if ((rc = round.run<NO_RERANK>())) return rc;
            const Refined &rf = round.rf;
            if ((rc = rr_count<false>(rf.keys, L.U, L.m, nullptr, 0, nullptr, w.ft_cnt, w.ft_head))) return rc;
            if ((rc = rr_scan(L.m, w.ft_cnt, w.ft_head, w.total + 4))) return rc;
            RrApply a = round_args(rf);
            a.tile_cnt = w.ft_cnt; a.tile_head = w.ft_head; a.tile_total = w.total + 4;
            a.has_isa = w.surv_bits; a.pair_v = w.surv_cnt;
            if ((rc = rr_apply<false, true, 4>(rf.keys, a))) return rc;
        }
        PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.surv_cnt, w.thead, tiles, w.total));
        uint32_t m32 = 0;
        { const int rcw = read_words(&m32, w.total, 4, st); if (rcw) return rcw; }
        L.m = m32;
        L.U = w.U0; L.G = w.G0; L.V = w.valsA; L.Un = w.U1; L.Gn = w.G1;
        if (L.m > 0)
            PROF(KC_RR_APPLY, n, st, hipLaunchKernelGGL((k_surv_compact), dim3((unsigned)tiles), dim3(256), 0, st, (const uint32_t *)w.surv_bits,
                                                        (const uint32_t *)surv_head, (const uint32_t *)SA, n, (const uint32_t *)w.surv_cnt,
                                                        (const uint32_t *)w.total, L.U, L.G, L.V));
        *first = FirstRound::FUSED64;
        T.ready = true;
        T.depth += T.s_sym;
        local.text_rounds++;
        local.rounds++;
        if (trace) fprintf(stderr, "suffix_array_amd: text round %d depth %lld: tied %lld -> %lld  (%.2f ms)\n", local.text_rounds, (long long)T.depth, (long long)tied0, (long long)L.m, lap());
        return SA_AMD_OK;
    }

    // 4. group heads of the initial order: how many suffixes are still tied (read-back: that count).  *tnext_scanned: w.tnext was
    // scanned here with the counts (k_rr_scan_round), the rank set-up launches no k_rr_scan_next
    int group_heads(const Route &R, const InitialOrder &O, int64_t tiles, bool *tnext_scanned)
    {
        int rc;
        // (64-bit keys: also every tile's first group start: the dense route's first ranks are tail ranks, k_rr_apply FTAIL)
        rc = R.top_shift ? rr_count<true, uint32_t>(O.sorted32, nullptr, n)
           : O.head_flags ? rr_count<true, uint64_t, true, true>((const uint64_t *)O.sr.keys, nullptr, n, w.tnext, 0, nullptr, nullptr, nullptr, O.head_flags)
                          : rr_count<true, uint64_t, true>((const uint64_t *)O.sr.keys, nullptr, n, w.tnext);
        if (rc) return rc;
        // (64-bit keys on a route that is expected to be dense -- Route::dense_expected, which the flags pass is chosen by too: the
        // tiles' next group starts are scanned here, as the second block of the launch, not by a launch of their own in front of the
        // rank set-up.  The read-back below waits for both blocks, so the launch is as long as the longer scan -- at C3 size 51 us
        // for this block against 32 us for k_rr_scan alone: the dense route saves k_rr_scan's 32 us and a launch.  Any other route
        // keeps the plain scan; should it turn dense after all, the rank set-up launches k_rr_scan_next itself)
        *tnext_scanned = !R.top_shift && R.dense_expected();
        if (*tnext_scanned)
            PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan_round), dim3(2), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total, w.tnext,
                                                           (uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr));
        else if ((rc = rr_scan(n))) return rc;
        uint32_t m32 = 0;
        { const int rcw = read_words(&m32, w.total, 4, st); if (rcw) return rcw; }
        L.m = m32;
        local.unresolved_after_initial = L.m;
        if (timing_only()) L.m = 0;   // diag library: ablation kernels produce wrong orders; stop here
        return SA_AMD_OK;
    }

    // the suffixes tied on the top 32 key bits are ordered by their low key bits: the initial sort is finished (read-back: tied on all 64 bits)
    int finish_top32_ties(const Route &R, const InitialOrder &O, ListState &T)
    {
        int rc;
        if (!R.top_shift || L.m <= 0) return SA_AMD_OK;
        L.keys_beside(w, O.sr.keys);
        if ((rc = rr_apply<true, false, 1, uint32_t>(O.sorted32, first_args(0u, w.has_isa)))) return rc;
        KeySrc K = KeySrc(); K.mode = KS_LOWKEY; K.kb = R.top_shift;
        RefineRound round(*this, R.Pp, K, rs);
        if ((rc = round.run<NO_RERANK>())) return rc;
        const Refined &rf = round.rf;
        if ((rc = rr_count<false>(rf.keys, L.U, L.m))) return rc;
        if ((rc = rr_scan(L.m))) return rc;
        if ((rc = rr_apply<false, true, 3>(rf.keys, round_args(rf)))) return rc;
        uint32_t m32 = 0;
        { const int rcw = read_words(&m32, w.total, 4, st); if (rcw) return rcw; }
        L.m = m32;
        L.advance(rf);
        T.ready = true;
        local.unresolved_after_initial = L.m;           // now: tied on the whole 64-bit key, as after a full sort
        return SA_AMD_OK;
    }

    // 5. dense route: ranks + ISA; otherwise compaction and the text-keyed rounds (read-back per round: tied count)
    int rank_setup_and_text_rounds(const Route &R, InitialOrder &O, ListState &T, bool tnext_scanned, RankSetup *setup)
    {
        int rc;
        const SortResult<uint64_t> &sr = O.sr; const int64_t tiles = T.tiles;
        // 5. refinement of the tied suffixes.  Three regimes:
        //   text rounds  while more than n / SPARSE_DIV suffixes are tied: secondary key = the next symbols of
        //                the text itself (no rank array needed yet), depth grows by s symbols per round;
        //   sparse       few tied suffixes: prefix doubling, ranks looked up without an ISA (sparse_key2);
        //   dense        prefix doubling with a full ISA (repetitive texts, or forced for A/B measurements).
        key2_bits = bit_length((uint64_t)(2 * n));
        const int64_t sparse_div = tn.sparse_div;      // (SA_AMD_SPARSE_DIV moves the boundary for tests / A-B)
        const int64_t sparse_limit = n / sparse_div;
        // (dense_expected without force_dense: only while more suffixes are tied than the sparse rounds take)
        const bool dense_first = L.m > 0 && !T.ready && (R.force_dense || (R.dense_expected() && L.m > sparse_limit));
        if (dense_first) {
            // ranks (ISA scatter) + compaction of the tied suffixes; SA already holds the sorted order
            // the first ranks are TAIL ranks (a group's last slot + 1), the form the dense rounds keep (k_rr_apply): the first doubling
            // round then writes only the ranks that change (SA_AMD_NO_FIRST_TAIL=1: head ranks, everything rewritten in round 1)
            const bool isa_tail_ranks = setup->isa_tail_ranks = !tn.no_first_tail;
            if (isa_tail_ranks && !tnext_scanned)
                PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan_next), dim3(1), dim3(SPINE_THREADS), 0, st, w.tnext, tiles, (uint32_t *)nullptr));
            RrApply a = first_args((uint32_t)n);
            a.tile_next = isa_tail_ranks ? w.tnext : (uint32_t *)nullptr;
            if (binned(n, n, tn)) {
                uint64_t *pk = (sr.keys == w.keysA) ? w.keysB : w.keysA;
                // the pairs are (SA[i], rank of slot i): k_rr_apply writes only the ranks and the binning reads its keys from the suffix
                // array itself, dSA[0 .. n] with the sentinel n in front (skipped by the scatter, as in the inverse permutation of the
                // text-round route) -- 4n bytes less written than a copy of SA.  The 64-bit buffers serve as two halves of n + 1 32-bit
                // entries each: ranks at pk[H + 1 ..], pass 1 -> sr.keys (dead once k_rr_apply has read it), pass 2 -> pk.
                // (Tuning::setup_key_copy, diagnostic library: k_rr_apply copies SA into the pairs' keys, as before)
                const bool from_sa = !tn.setup_key_copy && (((uintptr_t)dSA) & 15) == 0;
                const size_t H = ((size_t)n + 1 + 3) & ~(size_t)3;
                uint32_t *pk32 = (uint32_t *)pk, *sk32 = (uint32_t *)sr.keys;
                uint64_t *pk_out = from_sa ? (uint64_t *)nullptr : pk;
                uint32_t *pv_out = from_sa ? pk32 + H + 1 : w.U1;
                a.pair_k = pk_out; a.pair_v = pv_out;
                if ((rc = rr_apply_setup<2>(O, isa_tail_ranks, a))) return rc;
                if (from_sa) {
                    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, dSA, (uint32_t)n);
                    LAUNCH_CHECK(st);
                    rc = scatter_binned(w.ss, w.isa, dSA, pk32 + H, sk32, sk32 + H, n + 1, n, st, &local, tn, false, pk32);
                } else
                    rc = scatter_binned(w.ss, w.isa, (uint32_t *)pk, w.U1, (uint32_t *)sr.keys, w.G1, n, n, st, &local, tn);
                if (rc) return rc;
            } else if ((rc = rr_apply_setup<0>(O, isa_tail_ranks, a))) return rc;
        } else if (L.m > 0) {
            // compaction only; the sorted initial keys stay intact for the rank look-ups
            if ((rc = rebuild_sorted_keys(R, O))) return rc;
            HIP_TRY(hipMemsetAsync(w.has_isa, 0, ((size_t)n + 31) / 32 * 4, st));
            if (!T.ready) {
                L.keys_beside(w, sr.keys);
                if ((rc = rr_apply<true, false, 1>((const uint64_t *)sr.keys, first_args(0u, w.has_isa)))) return rc;
            }
            // ---- text-keyed rounds ----
            bool progressing = true;     // a text round that resolves little (runs, long repeats) is the last one
            while (R.text_ok && T.s_sym > 0 && L.m > sparse_limit && local.text_rounds < tn.max_text_rounds && progressing) {
                if ((rc = early_maybe_start())) return rc;
                const int64_t m_before = L.m;
                KeySrc K = KeySrc(); K.mode = KS_TEXT; K.h = T.depth; K.s = T.s_sym; K.kb = T.tkb;
                // (deferred: one read-back per round while the rounds have nothing for the global sort)
                RefineRound round(*this, T.Ptext, K, rs, rs.prev_clean && rs.local_ok && !tn.no_defer);
                if ((rc = round.run<3>())) return rc;
                after_round(round);
                T.depth += T.s_sym;
                local.text_rounds++;
                progressing = L.m * 4 <= m_before * 3;
                if (trace) fprintf(stderr, "suffix_array_amd: text round %d depth %lld: tied %lld -> %lld  (%.2f ms)\n", local.text_rounds, (long long)T.depth, (long long)m_before, (long long)L.m, lap());
            }
            if (L.m > sparse_limit) {
                // still many ties (repetitive text): build the ISA of the current order and double densely
                if (binned(n, n, tn) && (((uintptr_t)dSA) & 15) == 0) {
                    // inverse permutation without n random 4-byte stores: dSA[0 .. n] itself is the key array (dSA[0] = n, the
                    // sentinel, is skipped by the scatter), the value is the index = rank; one 32-bit radix pass bins the pairs by
                    // the top 8 bits of the suffix position, the scatter then works window by window (10.0 -> ~2.5 ms at 256 MiB)
                    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, dSA, (uint32_t)n);
                    LAUNCH_CHECK(st);
                    const size_t H = ((size_t)n + 1 + 3) & ~(size_t)3;      // keys in the first half of an 8(n + 64)-byte buffer, values in the second
                    rc = scatter_binned(w.ss, w.isa, dSA, nullptr, (uint32_t *)L.rkB, (uint32_t *)L.rkB + H, n + 1, n, st, &local, tn, true,
                                        (uint32_t *)L.rkA, (uint32_t *)L.rkA + H);
                    if (rc) return rc;
                } else
                    PROF(KC_SCATTER, n, st, hipLaunchKernelGGL((k_isa_from_sa), dim3(capped_grid(n, 256, 16384)), dim3(256), 0, st, (const uint32_t *)SA, w.isa, n));
                PROF(KC_SCATTER, L.m, st, hipLaunchKernelGGL((k_isa_tied), dim3(capped_grid(L.m, 256, 16384)), dim3(256), 0, st, (const uint32_t *)L.V,
                                                           (const uint32_t *)L.G, w.isa, L.m, n));
            } else {
                setup->sparse = L.m > 0;
            }
        }
        local.sparse_mode = setup->sparse ? 1 : 0;
        if (trace) fprintf(stderr, "suffix_array_amd: initial sort + text rounds + rank set-up done, %lld tied (%.2f ms since the last line)\n", (long long)L.m, lap());
        return SA_AMD_OK;
    }

    // prefix doubling on what is still tied, dense (ISA) or sparse (read-backs per round: tied count, ranks written)
    int doubling_rounds(const Route &R, const InitialOrder &O, int64_t depth, const RankSetup &setup)
    {
        int rc;
        // `depth` symbols are sorted, so the first offset is `depth`
        const int64_t depth_text = depth;
        int64_t h = depth;
        const bool sparse = setup.sparse;
        rs.parent_tail = setup.isa_tail_ranks;
        rs.changed_prev = setup.isa_tail_ranks ? L.m : 0;
        rs.m_local_off = L.m;
        rs.counters_clear = false;      // (the first doubling round zeroes the big-group counters itself, whatever the text rounds left)
        while (L.m > 0) {
            if (local.rounds >= 48) return SA_AMD_EINTERNAL;
            if ((rc = early_maybe_start())) return rc;     // (every slot outside the tied list is final from here on)
            const int64_t m_before = L.m;
            // the same refinement machinery as the text rounds, keyed by ranks.  Dense: ranks from the ISA; sparse: looked up without one (sparse_key2)
            KeySrc K = KeySrc();
            K.mode = sparse ? KS_SPARSE : KS_RANK; K.h = h; K.kb = key2_bits; K.isa = w.isa;
            K.has_isa = w.has_isa; K.sorted_keys = O.sr.keys; K.sorted_top32 = O.sorted32; K.sa = SA; K.depth = depth_text; K.top_shift = R.top_shift;
            // the local pass was given up because (nearly) every member sat in a group no tile can own: it is tried again when the list has
            // halved, and every third round if the round then finds the average group small enough (RefineRound::decide_local; large lists
            // count their groups anyway; a Fibonacci word's groups shrink while the list does not, a periodic text's never do)
            if (!rs.local_ok && !tn.no_local_sort && L.m * 2 < rs.m_local_off) rs.local_ok = true;
            const bool retry_local = !rs.local_ok && ++rs.rounds_local_off >= 3;
            if (rs.local_ok) { rs.m_local_off = L.m; rs.rounds_local_off = 0; }
            // dense rounds chase (up to `chase` rank look-ups per member inside one launch) once a round has had no group left
            // for the global sort: from then on every surviving group is known to share (iters + 1) * h symbols
            K.iters = (!sparse && rs.local_ok && rs.chase_ok) ? (L.m >= tn.chase_big_min ? tn.chase_big : tn.chase) : 1;
            if (K.iters > 1) K.mode = KS_CHASE;
            // binned or direct ISA stores: by the number of ranks this round is expected to write -- all of them when the parents'
            // ranks are not tail ranks yet, otherwise about as many as the round before wrote
            const int64_t expect = (!rs.parent_tail || L.m < rs.changed_prev) ? L.m : rs.changed_prev;
            const bool bin = !sparse && binned(n, expect, tn);
            // read-backs: a round whose predecessor had nothing for the global sort defers that question and blocks ONCE
            RefineRound round(*this, R.Pp, K, rs, rs.prev_clean && !bin && rs.local_ok && !tn.no_defer, true, retry_local);
            if ((rc = sparse ? round.run<1, false>() : bin ? round.run<2, true>() : round.run<0, true>())) return rc;
            const Refined &rf = round.rf;
            if (retry_local && rf.m_global < L.m) { rs.m_local_off = L.m; rs.rounds_local_off = 0; }      // (the local pass ran again; such a round is never deferred)
            if (round.missed) ++rs.deferred_misses;
            after_round(round);
            if (rs.prev_clean && (round.big_listed == 0 || m_before <= GS_CAP)) rs.all_small = true;
            if (!sparse) { rs.changed_prev = chg_sum(round.words); rs.parent_tail = true; }
            if (trace) fprintf(stderr, "suffix_array_amd: doubling round %d h %lld (%s, %d look-ups, %lld through the global sort): tied %lld -> %u, %lld ranks written\n", local.rounds, (long long)h, sparse ? "sparse" : "dense", K.iters, (long long)rf.m_global, (long long)m_before, round.words[RC_TIED], sparse ? -1ll : (long long)rs.changed_prev), fprintf(stderr, "    (%.2f ms)\n", lap());
            if (trace && !sparse) fprintf(stderr, "    (group starts read from %s)\n", rf.status ? "status bytes" : "keys");
            // every group that is still tied went through K.iters look-ups -- unless some went through the global sort (one look-up)
            h *= (K.iters > 1 && rf.m_global == 0) ? (int64_t)(K.iters + 1) : 2;
            rs.chase_ok = rf.m_global == 0;
        }
        return SA_AMD_OK;
    }

    // what a round of either loop leaves behind: the next tied list, and what the next round's switches are made from
    void after_round(const RefineRound &r)
    {
        rs.prev_clean = r.m_flagged == 0;
        rs.counters_clear = true;                     // (k_rr_scan_round ran ungated in the end)
        L.m = r.words[RC_TIED];
        L.advance(r.rf);
        local.rounds++;
    }

};

static int build_device(const uint8_t *dT, uint32_t *dSA, int32_t n32, void *dWork, int64_t work_bytes, hipStream_t st,
                        sa_amd_stats *stats, EarlyDownload *early = nullptr,
                        void *dWork2 = nullptr, int64_t work2_bytes = 0)      // reduced-memory route: the slabs that do not fit work_bytes live here (device-visible pinned host memory)
{
    const int64_t n = n32;
    DeviceBuild B;
    B.dT = dT; B.dSA = dSA; B.SA = dSA + 1; B.n = n; B.st = st;
    B.early = early;
    B.tn = route_tuning();
    B.trace = env_int("SA_AMD_VERBOSE", 0, 0, 9) >= 3;      // one line per refinement round on stderr
    B.trace_t = now_ms();
    memset(&B.local, 0, sizeof(B.local));
    g_readbacks = 0;
    const Tuning &tn = B.tn;
    sa_amd_stats &local = B.local;
    if (n == 0) {
        PROF(KC_MISC, 1, st, hipLaunchKernelGGL((k_set_u32), dim3(1), dim3(1), 0, st, dSA, 0u));
        HIP_TRY(hipStreamSynchronize(st));
        if (stats) *stats = local;
        return SA_AMD_OK;
    }
    B.w = dWork2 ? carve(dWork, n, (size_t)work_bytes, dWork2) : carve(dWork, n);
    const Workspace &w = B.w;
    if ((int64_t)w.bytes > work_bytes || (int64_t)w.bytes2 > work2_bytes) return SA_AMD_EINVAL;
    B.flags_slab_ok = !dWork2 || ((char *)w.keysC >= (char *)dWork && (char *)w.keysC + n <= (char *)dWork + work_bytes);
    if (n <= tn.small_max) {
        // small texts: the whole construction in one launch of one workgroup, everything in LDS (kernels/small.hpp)
        if (n <= SM_LITE_SINGLE_N)
            PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_small_sa_lite), dim3(1), dim3(SM_LITE_THREADS), 0, st, dT, dSA, (int)n, w.total));
        else
            PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_small_sa), dim3(1), dim3(SM_THREADS), 0, st, dT, dSA, (int)n, w.total));
        uint32_t rounds = 0;
        { const int rcw = read_words(&rounds, w.total, 4, st); if (rcw) return rcw; }
        local.rounds = (int)rounds;
        local.readbacks = g_readbacks;
        g_prof.resolve();
        g_last_stats = local;
        if (stats) *stats = local;
        return SA_AMD_OK;
    }
    HIP_TRY(hipMemsetAsync(w.ss.err, 0, 16, st));          // look-back give-ups of the single-pass scatter: checked at the end
    int rc;
    Route R;
    if ((rc = B.geometry_and_probes(R))) return rc;
    if (!R.unary) {
        InitialOrder O; ListState T; RankSetup ranks;
        FirstRound first = FirstRound::NONE; bool tnext_scanned = false;
        if ((rc = B.initial_sort(R, O))) return rc;
        B.open_lists(R, T);
        if ((rc = B.fast_finish32(R, O, T, &first))) return rc;
        if ((rc = B.fused_first_text_round(R, O, T, &first))) return rc;
        if (first == FirstRound::NONE) {      // (else the tied list is counted, and listed unless it is empty)
            if ((rc = B.group_heads(R, O, T.tiles, &tnext_scanned))) return rc;
            if ((rc = B.finish_top32_ties(R, O, T))) return rc;
        }
        if ((rc = B.rank_setup_and_text_rounds(R, O, T, tnext_scanned, &ranks))) return rc;
        if ((rc = B.doubling_rounds(R, O, T.depth, ranks))) return rc;
    }
    if ((rc = B.early_finish())) return rc;
    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, dSA, (uint32_t)n);   // reference src/saca.rs:13
    LAUNCH_CHECK(st);
    {
        // (synchronises the stream) a look-back that gave up means a tile scatter wrote nothing useful: never a silent wrong array
        // (word 3: a bucket larger than the shape the host picked for k_bucket_sort)
        uint32_t gave_up[4] = { 0, 0, 0, 0 };
        const int rcw = read_words(gave_up, w.ss.err, 16, st); if (rcw) return rcw;
        if (gave_up[0] || gave_up[3]) return SA_AMD_EINTERNAL;
    }
    local.readbacks = g_readbacks;
    if (B.trace) fprintf(stderr, "suffix_array_amd: %d blocking read-backs in this build (%d rounds deferred their mid-round count and had to run the global sort after all)\n", g_readbacks, B.rs.deferred_misses);
    g_prof.resolve();
    g_last_stats = local;
    if (stats) *stats = local;
    return SA_AMD_OK;
}

}  // namespace sa
