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
    w.surv_cnt = (uint32_t *)take(rr_tiles * 4);          // (not tcnt: refine_list uses that one for its own compaction)
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

struct Refined {
    const uint64_t *keys; const uint32_t *vals; uint32_t *vnext;
    int64_t m_global;                      // members ordered by the global sort
    const uint8_t *status = nullptr;       // != nullptr: the round's status bytes (RS_*, kernels/common.hpp) -- the re-rank reads the group starts from them, `keys` holds true keys at RS_KEYED places only
};

// Read-backs of a refinement round (DeviceBuild::finish_round).  A round used to block twice: once in the middle for the number
// of members the local pass could not order (they go through the global sort before the re-rank) and once at its end for the
// number still tied.  From the second round of a kind on nearly every round has NO such members, so the caller may ask
// refine_list to DEFER the first question: the local pass and its counting kernels are launched, the count stays on the device
// (w.total[RC_FLAGGED]) and the re-rank kernels behind it are launched GATED on it -- they do nothing when it is not zero.
// One read-back at the end of the round then answers both; in the rare round that did have such members the caller calls
// refine_list again with the words it read (resume_tot), which runs the global sort of those members, and launches the
// re-rank kernels ungated.
constexpr int RC_FLAGGED = 16, RC_GROUPS = 8, RC_BIG_LISTED = 12, RC_BIG_ORDERED = 13, RC_WORDS = 17;      // words of w.total
constexpr int RC_BIG_LISTED_SAVED = 14, RC_BIG_ORDERED_SAVED = 15;     // ... where k_rr_scan_round puts the two big-group counters before it zeroes them for the next round
constexpr int RC_BIG_CLASS = 17;       // ... and [17], [18]: the lengths of the two lists k_big_classify sorts the listed heads into; zeroed with the two counters
static_assert(RC_BIG_CLASS == RC_BIG_LISTED + RR_CLEAR_CLASS && RC_BIG_CLASS + 2 <= 64, "k_rr_scan_round zeroes them relative to the big-group counters; w.total has 64 words");
struct RoundCtl {
    bool defer = false;                    // in: do not read the local pass's counts back, return right behind its launches
    const uint32_t *resume_tot = nullptr;  // in: the counts (RC_WORDS words of w.total) of a deferred call that did have flagged members
    bool skip_big = false;                 // in: no group can be larger than GS_CAP any more: k_group_sort_big is not launched
    bool counters_clear = false;           // in: the previous round's k_rr_scan_round has zeroed w.total[RC_BIG_LISTED .. +1]
    bool deferred = false;                 // out: the counts were left on the device
    int64_t m_flagged = -1;                // out: members the local pass left to the global sort (-1: no local pass ran)
    int64_t big_listed = -1;               // out: groups listed for k_group_sort_big (-1: not looked for)
    bool missed = false;                   // out (finish_round): the deferred count was not zero, the global sort ran after all
};

// The tied list: the m suffixes that still share their rank with a neighbour, in slot order.  A refinement round reads
// (U, G, V), uses the next buffers as scratch, and the re-rank writes the next list into (Un, Gn, rf.vnext).
struct TiedList {
    uint32_t *U = nullptr, *G = nullptr, *V = nullptr;       // per member: its slot in SA, the first slot of its group, the suffix
    uint32_t *Un = nullptr, *Gn = nullptr;
    uint64_t *rkA = nullptr, *rkB = nullptr;                 // key buffers of the refinement rounds
    int64_t m = 0;
    void advance(const Refined &rf) { std::swap(U, Un); std::swap(G, Gn); V = rf.vnext; }
    uint32_t *valt(const Workspace &w) const { return V == w.valsA ? w.valsB : w.valsA; }
    // the sorted initial keys stay where they are (rank look-ups): the rounds take the two key buffers beside them
    void keys_beside(const Workspace &w, const uint64_t *initial) { rkA = initial == w.keysA ? w.keysB : w.keysA; rkB = w.keysC; }
};

// The arguments of k_rr_apply (kernels/rerank.hpp) by name, each defaulting to "not used"; DeviceBuild::rr_apply launches it.
struct RrApply {
    const uint32_t *V = nullptr, *U = nullptr;               // U == nullptr: element i sits in slot i
    int64_t m = 0;
    const uint32_t *tile_cnt = nullptr, *tile_head = nullptr, *tile_total = nullptr;     // nullptr: the workspace's tcnt, thead, total
    uint32_t *SA = nullptr, *ISA = nullptr, *Uo = nullptr, *Go = nullptr, *Vo = nullptr, n_text = 0;
    uint32_t *has_isa = nullptr, *pair_v = nullptr, *changed_cnt = nullptr;
    uint64_t *pair_k = nullptr;
    const uint32_t *tile_next = nullptr, *gate = nullptr;
    int g_shift = 0, key_shift = 0, parent_tail = 0, sa_final = 0;
    const uint8_t *status = nullptr;                         // a round behind a local pass that wrote status bytes (Refined::status)
};

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

// One device-resident build, phase by phase.  The members are what the phases hand to each other; every phase returns an
// SA_AMD_* status.  The blocking 4-byte read-backs that steer the host (how many suffixes are still tied, how many groups,
// how many ranks changed) are the read_words calls inside the phases: each one names what it reads.
struct DeviceBuild {
    // ---- inputs ----
    const uint8_t *dT;
    uint32_t *dSA, *SA;                 // SA = dSA + 1: the n sorted suffixes behind the sentinel slot
    int64_t n;
    hipStream_t st;
    Tuning tn;
    Workspace w;
    sa_amd_stats local;
    EarlyDownload *early = nullptr;     // host-pointer callers: the array starts travelling before the last rounds are done
    bool trace = false;
    double trace_t = 0;
    double lap() { const double t = now_ms(), d = t - trace_t; trace_t = t; return d; }
    bool timing_only() const            // diag library only: stop after the initial sort (array NOT finished)
    {
#ifdef SA_AMD_DIAG
        return tn.timing_only_initial_sort;
#else
        return false;
#endif
    }
    // ---- key geometry and route (geometry_and_probes) ----
    KeyParams P, Ptext;
    int sigma = 0, key_bits = 0, g_bits = 0, top_shift = 0;
    bool force_dense = false, text_ok = false, local_ok = false, probe_dense = false;
    // ---- initial order (initial_sort) ----
    SortResult<uint64_t> sr;
    const uint32_t *sorted32 = nullptr; // top-32 stage: the sorted 32-bit keys (no 64-bit sorted array exists)
    int bucket_top_bits = 0;            // key bits the two global passes in front of the bucket sort order (0: four global passes)
    bool flat_text = false;             // short text whose byte values are equally frequent: narrower initial keys (geometry_and_probes)
    bool bucket_finished = false;       // ... and k_bucket_sort has already ordered the suffixes tied on those 32 bits by their low key bits
    uint64_t *sorted0 = nullptr;        // the initial keys in SA order (kept for the rank look-ups)
    // Group-start flags (kernels/common.hpp, OS_HF_*): != nullptr: the last pass of the 64-bit initial sort wrote one flag byte per
    // slot here instead of the sorted keys, and sr.keys holds true keys only at the ends of that pass's digit runs.  The first
    // re-rank (group_heads, the rank set-up of the dense route) reads the flags; every other reader of the sorted keys gets them
    // rebuilt first (rebuild_sorted_keys).  The flags live in w.keysC, which nothing else touches between the last sort pass and
    // the end of the first k_rr_apply.
    uint8_t *head_flags = nullptr;
    bool flags_slab_ok = true;          // w.keysC is device memory (reduced-memory route: it may be the pinned host block -- then the key route is taken)
    // ---- the tied list and its buffers (from first_round_from_sorted_keys on) ----
    TiedList L;
    int64_t tiles = 0, depth = 0;       // tiles: RR_TILE-element tiles of the whole array (the re-rank steps straight from the initial order)
    uint32_t m32 = 0;
    bool lists_ready = false, finished32 = false, fused64 = false, sparse = false;
    bool isa_tail_ranks = false;        // the rank set-up of the dense route wrote tail ranks (k_rr_apply FTAIL)
    int s_sym = 0, tkb = 0, key2_bits = 0;
    bool unary_done = false;            // a text of one byte value: the array was written directly (geometry_and_probes), nothing else runs
    bool prev_clean = true;             // the last refinement round's local pass ordered every member (optimistic for the first one: a miss costs three empty launches)
    int deferred_misses = 0;            // rounds that deferred their mid-round read-back and did have members for the global sort (RoundCtl)

    // Early download: called wherever (L.U, L.m) is the current tied list and every slot outside it is final
    int early_maybe_start()
    {
        if (!early || early->started || L.m <= 0 || L.m > early->threshold || !early->start) return SA_AMD_OK;
        if (!early->ev && hipEventCreateWithFlags(&early->ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return SA_AMD_OK; }
        hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, dSA, (uint32_t)n);   // reference src/saca.rs:13 (the first chunk carries it)
        LAUNCH_CHECK(st);
        HIP_TRY(hipMemsetAsync(w.early_bits, 0, (((size_t)n + 1 + 31) / 32 + EARLY_THREADS) * 4, st));
        int64_t blocks = ceil_div(L.m, 256 * 8);
        if (blocks > 65536) blocks = 65536;
        if ((((uintptr_t)L.U) & 15) != 0) return SA_AMD_OK;       // (the list slabs are 256-byte aligned: cannot happen)
        PROF(KC_MISC, L.m, st, hipLaunchKernelGGL((k_early_mark), dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t *)L.U, L.m, (uint32_t)early->off, w.early_bits));
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
    int choose_bucket_bits() const
    {
        if (tn.no_bucket_sort || n < tn.bucket_min_n || n <= 1) return 0;
        const bool wide_ok = onesweep_on(w.ss, tn) && tn.onesweep32_shape == 0;      // (nine-bit digits: single-pass engine, default tile)
        if (tn.bucket_bits == 18 && wide_ok) return 18;
        if (tn.bucket_bits == 16) return 16;
        // (measured, random bytes and DNA: with the two key bits that travel in the values (initial_sort_top32) 18 bits win from about
        // 4.9e8 suffixes on -- 2^29: 9.09 against 9.36 ms --, without them only where 16 bits no longer fit)
        const bool value_bits = wide_ok && !tn.no_value_bits && !tn.no_text_keys && g_bits <= 30 &&
                                ((sigma == 256 && P.bits == 8) || (sigma == 4 && P.bits == 2 && !tn.no_packed_text));
        if (value_bits && (n >> 16) > 7500 && (n >> 18) * 10 <= bucket_cap_max() * 9) return 18;
        if ((n >> 16) * 10 <= bucket_cap(2) * 9) return 16;
        if (wide_ok && (n >> 18) * 10 <= bucket_cap_max() * 9) return 18;
        if ((n >> 16) * 10 <= bucket_cap_max() * 9) return 16;
        return 0;
    }

    bool flat_rule_applies() const { return n >= 2 && n < tn.top32_probe_min_n && n < ((int64_t)1 << 24) && !tn.no_flat_rule; }

    // ---- the re-rank step: k_rr_count, k_rr_scan (a round: k_rr_scan_round, finish_round), k_rr_apply (kernels/rerank.hpp) ----
    // One launcher each, over the RR_TILE-element tiles of m elements; tile_cnt / tile_head / total == nullptr: the workspace's.
    // FLAGS: the groups come from head_flags, not from the keys (the first re-rank behind a flags pass of the initial sort)
    // (a round: its status bytes, `status`)
    template <bool FIRST, typename KeyT = uint64_t, bool PARENTS = false, bool FLAGS = false>
    int rr_count(const KeyT *keys, const uint32_t *U, int64_t m, uint32_t *tile_first = nullptr, int g_shift = 0, const uint32_t *gate = nullptr,
                 uint32_t *tile_cnt = nullptr, uint32_t *tile_head = nullptr, const uint8_t *status = nullptr)
    {
        PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_rr_count<FIRST, KeyT, PARENTS, FLAGS>), dim3(rr_count_grid<FLAGS>(m)), dim3(RR_THREADS), 0, st, keys, U, m,
                                                    tile_cnt ? tile_cnt : w.tcnt, tile_head ? tile_head : w.thead, 0, tile_first, g_shift, gate,
                                                    FLAGS ? (status ? status : (const uint8_t *)head_flags) : (const uint8_t *)nullptr));
        return SA_AMD_OK;
    }
    int rr_scan(int64_t m, uint32_t *tile_cnt = nullptr, uint32_t *tile_head = nullptr, uint32_t *total = nullptr)
    {
        PROF(KC_RR_SCAN, ceil_div(m, RR_TILE), st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, tile_cnt ? tile_cnt : w.tcnt,
                                                                      tile_head ? tile_head : w.thead, ceil_div(m, RR_TILE), total ? total : w.total));
        return SA_AMD_OK;
    }
    template <bool FIRST, bool WRITE_SA, int ISA_MODE, typename KeyT = uint64_t, bool FTAIL = false, bool FLAGS = false>
    int rr_apply(const KeyT *keys, const RrApply &a)
    {
        PROF(KC_RR_APPLY, a.m, st, hipLaunchKernelGGL((k_rr_apply<FIRST, WRITE_SA, ISA_MODE, KeyT, FTAIL, FLAGS>), dim3((unsigned)ceil_div(a.m, RR_TILE)), dim3(RR_THREADS), 0, st,
                                                      keys, a.V, a.U, a.m, a.tile_cnt ? a.tile_cnt : (const uint32_t *)w.tcnt,
                                                      a.tile_head ? a.tile_head : (const uint32_t *)w.thead, a.SA, a.ISA, a.Uo, a.Go, a.Vo, a.n_text, a.has_isa, a.g_shift,
                                                      a.pair_k, a.pair_v, a.tile_total ? a.tile_total : (const uint32_t *)w.total, a.key_shift, a.tile_next,
                                                      a.parent_tail, a.changed_cnt, a.gate, a.sa_final,
                                                      FLAGS ? (a.status ? a.status : (const uint8_t *)head_flags) : (const uint8_t *)nullptr));
        return SA_AMD_OK;
    }
    // the rank set-up of the dense route (ISA_MODE 0: direct ISA stores, 2: ranks for the binned scatter): tail or head ranks,
    // groups from the flags or from the sorted keys
    template <int ISA_MODE>
    int rr_apply_setup(const RrApply &a)
    {
        const uint64_t *k = sr.keys;
        if (head_flags)
            return isa_tail_ranks ? rr_apply<true, false, ISA_MODE, uint64_t, true, true>(k, a) : rr_apply<true, false, ISA_MODE, uint64_t, false, true>(k, a);
        return isa_tail_ranks ? rr_apply<true, false, ISA_MODE, uint64_t, true>(k, a) : rr_apply<true, false, ISA_MODE>(k, a);
    }
    // Flags were emitted but the route that follows reads the sorted keys (compaction for the text rounds, rank look-ups of the
    // sparse rounds): sr.keys[i] = the initial key of suffix SA[i], by the device function those look-ups compare with.  Rare in
    // real use (the flags are asked for only when the dense route is expected) and dear: about 50 ms at 256 MiB with gram keys.
    int rebuild_sorted_keys()
    {
        if (!head_flags) return SA_AMD_OK;
        int64_t blocks = ceil_div(n, GK_THREADS);
        if (blocks > 65536) blocks = 65536;
        PROF(KC_GATHER, n, st, hipLaunchKernelGGL((k_keys_of_suffixes), dim3((unsigned)blocks), dim3(GK_THREADS), 0, st, dT, P, n, (const uint32_t *)SA, sr.keys));
        head_flags = nullptr;
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
    // ... and every re-rank of the tied list: the refined order in, the next list out
    RrApply round_args(const Refined &rf, RrApply a = RrApply()) const
    {
        a.V = rf.vals; a.U = L.U; a.m = L.m; a.SA = SA; a.ISA = w.isa; a.Uo = L.Un; a.Go = L.Gn; a.Vo = rf.vnext; a.n_text = (uint32_t)n;
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
        PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_count_sample_dups), dim3((unsigned)(ceil_div(S, 256) < 4096 ? ceil_div(S, 256) : 4096)), dim3(256), 0, st, (const uint64_t *)w.keysA, S,
                                                (unsigned long long *)w.keysB, H - 1u, w.total));
        return SA_AMD_OK;
    }
    // the 64-bit initial keys (plain or gram form) into w.keysA, with the first sort pass's digit counts when the sort wants them
    int build_keys64(uint32_t *vals0, uint8_t *packed_out, const FirstCounts &fc, bool counted)
    {
        const int nb0 = key_bits < RADIX_BITS ? key_bits : RADIX_BITS;
        const unsigned grid = (unsigned)ceil_div(ceil_div(n, KB_TILE), KB_TPW);
        PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((P.gram > 0 ? k_build_keys<false, true> : k_build_keys<false>), dim3(grid), dim3(KB_THREADS), 0, st, dT, n, P, w.keysA, vals0,
                                                      (uint32_t *)nullptr, 0, packed_out, counted ? fc.counts : (uint32_t *)nullptr, fc.chunk_elems, fc.G, (1u << nb0) - 1u, 0));
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

    // Three-way split of giant groups around their majority key (kernels/refine.hpp, k_split_*): the keys in L.rkA carry the dense
    // group index above bit kb, w.ft_cnt the exclusive group-start counts per tile.  *taken = false: the count pass found more
    // than an eighth of the members off their group's pivot key (or the scratch buffers too small) -- nothing has been changed,
    // the caller sorts the list with the radix sort.  L.Un / L.Gn: the list's next buffers, free until the re-rank.
    int split_giant_groups(uint32_t groups, int kb, int sort_bits, Refined *out, bool *taken,
                           bool starts_ready)            // the gather has written the table of group starts (first array in L.Gn)
    {
        const int64_t m = L.m;
        uint32_t *const Valt = L.valt(w);
        *taken = false;
        const int64_t tiles = ceil_div(m, RR_TILE);
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        char *sg = (char *)L.Gn;
        uint32_t *starts = (uint32_t *)sg;            sg += up(((size_t)groups + 1) * 4);     // list index of every group's first member (+ m)
        uint32_t *mps = (uint32_t *)sg;               sg += up(((size_t)groups + 1) * 4);     // minority members in front of it (+ their total)
        uint32_t *Lless = (uint32_t *)sg;             sg += up((size_t)groups * 4);           // minority members of the group below its pivot
        uint64_t *pivot = (uint64_t *)sg;             sg += up((size_t)groups * 8);
        const size_t cap = (size_t)m / 8 + 1;                                                  // (minority members when the split is taken)
        uint32_t *mv = (uint32_t *)sg, *mv_alt = mv + ((cap + 63) & ~(size_t)63);
        uint64_t *mk = (uint64_t *)L.Un, *mk_alt = mk + ((cap + 31) & ~(size_t)31);
        const size_t need_g = (size_t)(sg - (char *)L.Gn) + 2 * ((cap + 63) & ~(size_t)63) * 4;
        const size_t need_u = 2 * ((cap + 31) & ~(size_t)31) * 8;
        if (need_g > (size_t)n * 4 || need_u > (size_t)n * 4) return SA_AMD_OK;
        if (!starts_ready)
            PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_group_starts), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, L.U, L.G, m,
                                                        (const uint32_t *)w.ft_cnt, groups, starts));
        PROF(KC_MISC, groups, st, hipLaunchKernelGGL((k_split_pivots), dim3((unsigned)ceil_div((int64_t)groups, 256)), dim3(256), 0, st,
                                                 (const uint64_t *)L.rkA, (const uint32_t *)starts, groups, kb, pivot));
        PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_split_count), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, (const uint64_t *)L.rkA, m, kb,
                                                    (const uint64_t *)pivot, w.tcnt));
        PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total));
        uint32_t minor = 0;
        { const int rcw = read_words(&minor, w.total, 4, st); if (rcw) return rcw; }
        if ((int64_t)minor * 8 > m) return SA_AMD_OK;
        *taken = true;
        out->m_global = m;
        if (minor == 0) {                                  // every member carries its group's pivot key: the order stands
            out->keys = L.rkA; out->vals = L.V; out->vnext = Valt;
            return SA_AMD_OK;
        }
        PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((k_split_pass<false>), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st,
                                                    (const uint64_t *)L.rkA, (const uint32_t *)L.V, m, kb, (const uint64_t *)pivot,
                                                    (const uint32_t *)w.tcnt, (const uint32_t *)starts, groups, mps, (const uint32_t *)w.total,
                                                    mk, mv, (const uint32_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr));
        SortResult<uint64_t> s2;
        const int rc = sort_pairs(SortJob<uint64_t>{ mk, mv, mk_alt, mv_alt, minor, 0, sort_bits }, w.ss, st, tn, &s2, &local);
        if (rc) return rc;
        PROF(KC_MISC, groups, st, hipLaunchKernelGGL((k_split_less), dim3((unsigned)ceil_div((int64_t)groups, 256)), dim3(256), 0, st,
                                                 (const uint64_t *)s2.keys, (const uint32_t *)mps, (const uint64_t *)pivot, groups, kb, Lless));
        PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((k_split_pass<true>), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st,
                                                    (const uint64_t *)L.rkA, (const uint32_t *)L.V, m, kb, (const uint64_t *)pivot,
                                                    (const uint32_t *)w.tcnt, (const uint32_t *)starts, groups, mps, (const uint32_t *)w.total,
                                                    (uint64_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)Lless, L.rkB, Valt));
        PROF(KC_SCATTER, minor, st, hipLaunchKernelGGL((k_split_place_minor), dim3((unsigned)ceil_div((int64_t)minor, 256)), dim3(256), 0, st,
                                                       (const uint64_t *)s2.keys, (const uint32_t *)s2.vals, (int64_t)minor, kb,
                                                       (const uint32_t *)starts, (const uint32_t *)mps, (const uint32_t *)Lless, L.rkB, Valt));
        out->keys = L.rkB; out->vals = Valt; out->vnext = L.V;
        return SA_AMD_OK;
    }

    // Where a dense doubling round keeps its status bytes (RS_*, kernels/common.hpp; nullptr: the round takes the key route).
    // They cannot share L.Gn with the key form's flags: k_rr_apply writes the next list's group heads there while it reads them.
    // On the route that starts rank doubling straight from the initial order the rounds' key buffers are w.keysA / w.keysB and
    // w.keysC is dead -- the initial sort's group-start flags in it are consumed by the rank set-up, the early download takes it
    // only when the rounds are over (early_finish).  Behind text rounds w.keysC is a key buffer of the rounds (keys_beside),
    // and on the reduced-memory route it may be pinned host memory (flags_slab_ok): keys then.  One byte per member, m <= n.
    uint8_t *round_status_slab(const KeySrc &K) const
    {
        if (tn.round_flags == 0 || (K.mode != KS_RANK && K.mode != KS_CHASE)) return nullptr;
        if (!flags_slab_ok || L.rkA == w.keysC || L.rkB == w.keysC) return nullptr;
        return (uint8_t *)w.keysC;
    }

    // One refinement round of the tied list with a secondary key taken from the text (KeySrc): afterwards every
    // group is ordered by (group head << kb) | key2.  Small groups: gather fused with the in-LDS group sort
    // (k_group_sort); groups no tile owns, or everything when *use_local is off: plain gather + global radix sort.
    // L.Un / L.Gn: the list's next buffers, free until the re-rank.
    int refine_list(const KeyParams &Pk, const KeySrc &K_in, bool *use_local, Refined *out, bool retry_local = false,
                    int *split_rest = nullptr,        // rounds the three-way split sits out after its count pass found no majority
                    RoundCtl *ctl = nullptr)
    {
        const int64_t m = L.m;
        uint32_t *const Valt = L.valt(w);
        KeySrc K = K_in;
        K.net_min = tn.network_min;
        const bool resume = ctl && ctl->resume_tot;
        const int64_t tiles = ceil_div(m, RR_TILE);
        const int kb = K.kb;
        SortResult<uint64_t> sr;
        int rc;
        // sparse look-up: its own kernel, one suffix per thread (a chain of ~60 dependent loads each)
        auto gather_sparse = [&]() -> int {
            int64_t gblocks = ceil_div(m, GK_THREADS);
            if (gblocks > 8192) gblocks = 8192;
            PROF(KC_GATHER, m, st, hipLaunchKernelGGL((k_gather_textkey<KS_SPARSE>), dim3((unsigned)gblocks), dim3(GK_THREADS), 0, st,
                                                      (const uint32_t *)L.V, L.G, dT, Pk, m, n, K, L.rkA));
            return SA_AMD_OK;
        };
        // The local pass was given up because (nearly) every member sat in a group no tile can own.  Lists large enough for the
        // dense group index count their groups anyway: when the average group has come down to about what a tile can own
        // (a Fibonacci word's groups shrink while the list does not), the local pass is tried again -- in this round
        bool counted = false;
        uint32_t groups = 0;
        if (!*use_local && retry_local && !tn.no_local_sort && m < tn.dense_rekey_min) *use_local = true;     // (small lists do not count their groups)
        if (!*use_local && retry_local && !tn.no_local_sort && m >= tn.dense_rekey_min) {
            PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_flag_count<false>), dim3(rr_count_grid<false>(m)), dim3(RR_THREADS), 0, st,
                                                        (const uint8_t *)nullptr, L.U, L.G, m, w.tcnt, w.ft_cnt));
            PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.ft_cnt, w.thead, tiles, w.total + 8));
            { const int rcw = read_words(&groups, w.total + 8, 4, st); if (rcw) return rcw; }
            counted = true;
            if ((int64_t)groups * 2 * tn.group_cap >= m) *use_local = true;
        }
        const bool had_local_pass = *use_local;            // (then the keys are in L.rkA already when the whole list goes through the global sort after all)
        uint8_t *const status = round_status_slab(K);      // != nullptr: the local pass writes status bytes there and no keys for the members it orders
        out->status = nullptr;
        if (*use_local) {
            uint8_t *flags = status ? status : (uint8_t *)L.Gn;
            const unsigned gs_blocks = (unsigned)ceil_div(m, GS_TILE);
            const int cap = tn.group_cap;                    // largest group ordered in LDS (C3: 1024 beats 512 by 1%)
            // groups of up to GB_CAP (8 192) members whose keys fit 32 bits: one workgroup each, in LDS (k_group_sort_big), on the list of
            // their first members that k_group_sort writes (L.Un is free until k_flag_gather); the rest goes through the global sort
            const bool big_local = !tn.no_big_group_sort && kb <= 32 && m > GS_CAP && !(ctl && ctl->skip_big);
            uint32_t *bheads = big_local ? L.Un : (uint32_t *)nullptr, *bcount = big_local ? w.total + RC_BIG_LISTED : (uint32_t *)nullptr;
            if (!resume) {
            if (!(ctl && ctl->counters_clear)) {
                HIP_TRY(hipMemsetAsync(w.total + RC_BIG_LISTED, 0, 8, st));           // [12] listed first members, [13] members ordered by k_group_sort_big
                HIP_TRY(hipMemsetAsync(w.total + RC_BIG_CLASS, 0, 8, st));            // [17], [18] listed groups of either k_group_sort_big instance
            }
            if (K.mode == KS_SPARSE && (rc = gather_sparse())) return rc;      // (then the sort on those keys: KS_PRE)
            if (status && tn.round_flags == 2) {
                // (diag library: what the round does not write must not be read -- a poisoned entry that is read changes the result)
                HIP_TRY(hipMemsetAsync(L.rkA, 0xEE, (size_t)m * 8, st));
                HIP_TRY(hipMemsetAsync(status, 0xFF, (((size_t)m + 7) & ~(size_t)7) + 8, st));
            }
#define GS_LAUNCH(M, S) PROF(KC_LOCAL, m, st, hipLaunchKernelGGL((k_group_sort<M, S>), dim3(gs_blocks), dim3(GS_THREADS), 0, st, (const uint32_t *)L.V, L.G, L.U, dT, Pk, m, n, K, \
                                                            L.rkA, L.V, flags, cap, bheads, bcount))
            switch (K.mode) {
            case KS_TEXT: GS_LAUNCH(KS_TEXT, false); break;
            case KS_LOWKEY: GS_LAUNCH(KS_LOWKEY, false); break;
            case KS_RANK: if (status) GS_LAUNCH(KS_RANK, true); else GS_LAUNCH(KS_RANK, false); break;
            case KS_CHASE: if (status) GS_LAUNCH(KS_CHASE, true); else GS_LAUNCH(KS_CHASE, false); break;
            default: GS_LAUNCH(KS_PRE, false); break;      // (KS_SPARSE: the keys have just been gathered)
            }
#undef GS_LAUNCH
            if (gs_blocks > 1)
                PROF(KC_LOCAL, 0, st, hipLaunchKernelGGL((k_group_sort_straddle), dim3(gs_blocks - 1), dim3(GX_THREADS), 0, st, L.rkA, L.V, L.G,
                                                         L.U, m, flags, cap, K, n));
            if (big_local) {
                const int lo = cap > GS_CAP ? cap : GS_CAP;
                // The listed heads are classified once (k_big_classify) into one list per instance, behind the heads in L.Un.  A tile
                // lists at most two heads -- the group that runs on beyond it and one of more than GS_CAP members inside it --, so
                // the heads end before hcap and neither list can outgrow it (3 * hcap <= m <= n: m > GS_CAP).
                const uint32_t hcap = (2u * gs_blocks + 63u) & ~63u;
                uint32_t *const bsmall = bheads + hcap, *const blarge = bheads + 2 * (size_t)hcap, *const bclass = w.total + RC_BIG_CLASS;
                if (3 * (int64_t)hcap > n) return SA_AMD_EINTERNAL;
                PROF(KC_LOCAL, 0, st, hipLaunchKernelGGL((k_big_classify), dim3((unsigned)ceil_div((int64_t)hcap, GC_THREADS)), dim3(GC_THREADS), 0, st, (const uint32_t *)L.G, m, lo,
                                                         (const uint32_t *)bheads, (const uint32_t *)bcount, bsmall, blarge, hcap, bclass));
                PROF(KC_LOCAL, 0, st, hipLaunchKernelGGL((k_group_sort_big<256>), dim3((unsigned)(8 * cu_count())), dim3(256), 0, st, L.rkA, L.V, L.G, m, kb, lo,
                                                         (const uint32_t *)bsmall, (const uint32_t *)bclass, hcap, flags, w.total + RC_BIG_ORDERED));
                PROF(KC_LOCAL, 0, st, hipLaunchKernelGGL((k_group_sort_big<512>), dim3((unsigned)(4 * cu_count())), dim3(512), 0, st, L.rkA, L.V, L.G, m, kb,
                                                         lo > GB_CAP_SMALL ? lo : GB_CAP_SMALL, (const uint32_t *)blarge, (const uint32_t *)(bclass + 1), hcap, flags,
                                                         w.total + RC_BIG_ORDERED));
            }
            PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((status ? k_flag_count<true> : k_flag_count<false>), dim3(status ? rr_count_grid<true>(m) : rr_count_grid<false>(m)), dim3(RR_THREADS), 0, st,
                                                        (const uint8_t *)flags, L.U, L.G, m, w.tcnt, w.ft_cnt));
            // (flagged members -> w.total[RC_FLAGGED], flagged groups -> w.total[RC_GROUPS]; one launch)
            PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan_pair), dim3(2), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, w.total + RC_FLAGGED,
                                                           w.ft_cnt, (uint32_t *)nullptr, w.total + RC_GROUPS, tiles));
            }
            if (ctl && ctl->defer && !resume) {
                // the counts stay on the device: the caller launches the re-rank kernels gated on w.total[RC_FLAGGED] and reads everything at once
                ctl->deferred = true;
                out->keys = L.rkA; out->vals = L.V; out->vnext = Valt; out->m_global = 0; out->status = status;
                return SA_AMD_OK;
            }
            uint32_t tot9[RC_WORDS] = { 0 };                      // [RC_FLAGGED] flagged members, [RC_GROUPS] flagged groups, [RC_BIG_ORDERED] members k_group_sort_big ordered
            if (resume) memcpy(tot9, ctl->resume_tot, sizeof(tot9));
            else {
                const int rcw = read_words(tot9, w.total, sizeof(tot9), st); if (rcw) return rcw;
                }
            const int64_t m_big = tot9[RC_FLAGGED], m_big_local = tot9[RC_BIG_ORDERED];
            if (ctl) { ctl->m_flagged = m_big; ctl->big_listed = big_local ? (int64_t)tot9[RC_BIG_LISTED] : -1; }
            // the flagged members are sorted in the first `half` entries of L.rkB / Valt with the second half as the alternate
            // buffers: half is even (16-byte aligned 8-byte keys) and half + m_big never exceeds the n entries the slabs hold
            const size_t half = ((size_t)n / 2) & ~(size_t)1;
            if ((size_t)m_big <= half && half + (size_t)m_big <= (size_t)n) {
                if (m_big > 0) {
                    // groups no tile owns: global sort of (index of the group among them, key2), then back to their list positions
                    // (a text that is one long run has ONE such group: no index bits at all, four passes instead of eight)
                    const int idx_bits = bit_length((uint64_t)(tot9[RC_GROUPS] > 0 ? tot9[RC_GROUPS] - 1 : 0));
                    PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((status ? k_flag_gather<true> : k_flag_gather<false>), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st,
                                                                (const uint8_t *)flags, (const uint64_t *)L.rkA, (const uint32_t *)L.V, L.U, L.G, m,
                                                                (const uint32_t *)w.tcnt, (const uint32_t *)w.ft_cnt, kb, L.rkB, Valt, L.Un));
                    SortJob<uint64_t> big{ L.rkB, Valt, L.rkB + half, Valt + half, m_big, 0, kb + idx_bits };
                    big.may_skip = true;
                    rc = sort_pairs(big, w.ss, st, tn, &sr, &local);
                    if (rc) return rc;
                    PROF(KC_SCATTER, m_big, st, hipLaunchKernelGGL((k_scatter_back), dim3((unsigned)ceil_div(m_big, 256)), dim3(256), 0, st,
                                                                   (const uint64_t *)sr.keys, (const uint32_t *)sr.vals,
                                                                   (const uint32_t *)L.Un, L.G, kb, m_big, L.rkA, L.V));
                }
                out->keys = L.rkA; out->vals = L.V; out->vnext = Valt; out->m_global = m_big + m_big_local;      // (neither kind has been chased)
                out->status = status;
                local.locally_sorted += m - m_big;
                if (m_big * 2 > m) *use_local = false;           // mostly large groups: not worth another local pass
                return SA_AMD_OK;
            }
            if (m_big * 10 >= m * 9) *use_local = false;     // (nearly) the whole list sits in groups no tile can own (runs, periodic texts): the next rounds skip the local pass
            if (status) {
                // The global sort below wants a key for EVERY member and the places the local pass owned have none: the pass runs again
                // in its key form for those places alone (k_group_sort REFILL), on the order it left.  It changes nothing in that
                // order and writes the keys it would have written the first time -- after a chase the places of the final
                // subgroups, so no subgroups merge and the round's tied count is what the key route's is.  The keys of every
                // other place are where the first launch, k_group_sort_straddle and k_group_sort_big left them.  A tile without an
                // owned place -- all of them on a run or a periodic text, which is what comes here -- returns behind 2 KiB of bytes.
#define GS_REFILL(M) PROF(KC_LOCAL, m, st, hipLaunchKernelGGL((k_group_sort<M, false, true>), dim3(gs_blocks), dim3(GS_THREADS), 0, st, (const uint32_t *)L.V, L.G, L.U, dT, Pk, m, n, K, \
                                                            L.rkA, L.V, status, cap, (uint32_t *)nullptr, (uint32_t *)nullptr))
                if (K.mode == KS_CHASE) GS_REFILL(KS_CHASE); else GS_REFILL(KS_RANK);
#undef GS_REFILL
            }
        }
        // the whole list through the global sort.  Large lists are keyed by (index of the group in the list, key2) instead of
        // (28-bit slot of the group head, key2) when that saves radix passes: count the group heads first, then gather the keys in
        // that form (k_gather_keyed) or re-key the ones the local pass left (k_rekey_dense).  The head slots are not put back
        // after the sort: the re-rank kernels only compare neighbouring keys.
        int sort_bits = kb + g_bits;
        bool rekeyed = false;
        if (m >= tn.dense_rekey_min) {
            if (!counted || had_local_pass) {              // (the local pass has used the count arrays for its own compaction)
                PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_flag_count<false>), dim3(rr_count_grid<false>(m)), dim3(RR_THREADS), 0, st,
                                                            (const uint8_t *)nullptr, L.U, L.G, m, w.tcnt, w.ft_cnt));
                PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.ft_cnt, w.thead, tiles, w.total + 8));
                { const int rcw = read_words(&groups, w.total + 8, 4, st); if (rcw) return rcw; }
                }
            const int idx_bits = bit_length((uint64_t)(groups > 0 ? groups - 1 : 0));
            if (ceil_div(kb + idx_bits, RADIX_BITS) < ceil_div(kb + g_bits, RADIX_BITS)) {
                sort_bits = kb + idx_bits;
                rekeyed = true;
            }
        }
        const bool split_wanted = rekeyed && !tn.no_split && m >= tn.split_min && groups > 0 && (int64_t)groups * tn.split_group_min <= m &&
                                  !(split_rest && *split_rest > 0);
        bool starts_ready = false;
        if (had_local_pass) {
            if (rekeyed)
                PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((k_rekey_dense), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, L.rkA, L.U, L.G, m,
                                                            (const uint32_t *)w.ft_cnt, kb));
        } else if (K.mode == KS_SPARSE) {
            if ((rc = gather_sparse())) return rc;
            if (rekeyed)
                PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((k_rekey_dense), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, L.rkA, L.U, L.G, m,
                                                            (const uint32_t *)w.ft_cnt, kb));
        } else {
            const uint32_t *th = rekeyed ? (const uint32_t *)w.ft_cnt : (const uint32_t *)nullptr;
            // (when the three-way split may follow, the gather also writes its table of group starts: the first array in L.Gn)
            uint32_t *gs = split_wanted ? L.Gn : (uint32_t *)nullptr;
            starts_ready = gs != nullptr;
#define GK_LAUNCH(M) PROF(KC_GATHER, m, st, hipLaunchKernelGGL((k_gather_keyed<M>), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, (const uint32_t *)L.V, L.U, L.G, dT, Pk, m, n, K, \
                                                              th, L.rkA, gs, groups))
            switch (K.mode) {
            case KS_TEXT: GK_LAUNCH(KS_TEXT); break;
            case KS_LOWKEY: GK_LAUNCH(KS_LOWKEY); break;
            default: GK_LAUNCH(KS_RANK); break;
            }
#undef GK_LAUNCH
        }
        // Giant groups (runs, periodic texts, long repeats): all but a few members of a group carry the same key, so the few
        // are pulled out and sorted on their own and the rest only shifts (split_giant_groups) -- if its count pass finds that
        // they are few indeed; otherwise the radix sort below.
        if (split_rest && *split_rest > 0) --*split_rest;
        else if (split_wanted) {
            bool taken = false;
            rc = split_giant_groups(groups, kb, sort_bits, out, &taken, starts_ready);
            if (rc || taken) return rc;
            if (split_rest) *split_rest = 3;              // (a Fibonacci word's groups fall into parts of similar size round after round)
        }
        SortJob<uint64_t> whole{ L.rkA, L.V, L.rkB, Valt, m, 0, sort_bits };
        whole.may_skip = true;
        rc = sort_pairs(whole, w.ss, st, tn, &sr, &local);
        if (rc) return rc;
        out->keys = sr.keys; out->vals = sr.vals; out->m_global = m;
        out->vnext = (sr.vals == L.V) ? Valt : L.V;
        return SA_AMD_OK;
    }

    // The end of a refinement round, text-keyed or doubling (RoundCtl): re-rank the order refine_list left in rf -- gated while the
    // round's mid-round count is deferred --, read the round's words back (words[0]: members still tied) and, when the deferred
    // count was not zero (ctl.missed), resume refine_list with the words just read and re-rank ungated.  ISA_MODE / PARENTS: the
    // k_rr_apply / k_rr_count instantiation (3: text-keyed, 1: sparse, 0: dense, 2: dense with binned ISA stores -- never
    // deferred, its pairs are scattered behind the read-back); extra: the k_rr_apply arguments beside round_args() and the gate.
    template <int ISA_MODE, bool PARENTS>
    int finish_round(const KeyParams &Pk, const KeySrc &K, RoundCtl &ctl, Refined &rf, const RrApply &extra, uint32_t *words, size_t words_bytes,
                     bool retry_local, int *split_rest)
    {
        int rc;
        const int64_t tiles_m = ceil_div(L.m, RR_TILE);
        for (int attempt = 0; ; ++attempt) {
            const uint32_t *gate = ctl.deferred ? (const uint32_t *)(w.total + RC_FLAGGED) : (const uint32_t *)nullptr;
            // dense rounds: a group's rank is its last slot + 1 and a parent's last subgroup keeps it (k_rr_apply, TAIL); the tiles
            // then also need the first group start BEHIND them (k_rr_scan_next, second block of k_rr_scan_round)
            // (rf.status: the local pass wrote status bytes, the group starts are read from them -- dense rounds only)
            bool by_status = false;
            if constexpr (PARENTS) by_status = rf.status != nullptr;
            if constexpr (PARENTS) {
                if (by_status) rc = rr_count<false, uint64_t, true, true>(rf.keys, L.U, L.m, w.tnext, key2_bits, gate, nullptr, nullptr, rf.status);
            }
            if (!by_status) rc = rr_count<false, uint64_t, PARENTS>(rf.keys, L.U, L.m, PARENTS ? w.tnext : (uint32_t *)nullptr, PARENTS ? key2_bits : 0, gate);
            if (rc) return rc;
            // (second block: the tiles' next group starts and the changed-rank counters of a dense round, the big-group counters saved and zeroed)
            PROF(KC_RR_SCAN, tiles_m, st, hipLaunchKernelGGL((k_rr_scan_round), dim3(2), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles_m, w.total,
                                                             PARENTS ? w.tnext : (uint32_t *)nullptr, PARENTS ? w.chg : (uint32_t *)nullptr, w.total + RC_BIG_LISTED, gate));
            RrApply a = round_args(rf, extra);
            a.gate = gate;
            a.status = rf.status;
            if constexpr (PARENTS) {
                if (by_status) rc = rr_apply<false, true, ISA_MODE, uint64_t, false, true>(rf.keys, a);
            }
            if (!by_status) rc = rr_apply<false, true, ISA_MODE>(rf.keys, a);
            if (rc) return rc;
            // the one read-back of the round: w.total and, where asked for, the changed-rank counters behind it (w.chg)
            { const int rcw = read_words(words, w.total, words_bytes, st); if (rcw) return rcw; }
            if constexpr (ISA_MODE == 2) {
                // (only the ranks that change became pairs; their number is in the counters)
                int64_t pairs = 0;
                for (int c = 0; c < RR_CHG_COUNTERS; ++c) pairs += words[64 + c * 32];
                if (pairs > 0 && (rc = scatter_binned(w.ss, w.isa, (uint32_t *)a.pair_k, a.pair_v, (uint32_t *)rf.keys, (uint32_t *)rf.vals, pairs, n, st, &local, tn))) return rc;
            }
            if (!ctl.deferred) return SA_AMD_OK;
            if (words[RC_FLAGGED] == 0) {
                // as expected: the local pass ordered everything (what k_group_sort_big ordered was not chased: one look-up)
                ctl.m_flagged = 0;
                ctl.big_listed = ctl.skip_big ? -1 : (int64_t)words[RC_BIG_LISTED_SAVED];
                rf.m_global = words[RC_BIG_ORDERED_SAVED];
                local.locally_sorted += L.m;
                return SA_AMD_OK;
            }
            if (attempt > 0) return SA_AMD_EINTERNAL;
            ctl.resume_tot = words; ctl.defer = false; ctl.deferred = false;      // (refine_list copies them before anything is read back again)
            rc = refine_list(Pk, K, &local_ok, &rf, retry_local, split_rest, &ctl);
            ctl.resume_tot = nullptr;
            if (rc) return rc;
            ctl.missed = true;
        }
    }

    // 1-2. which byte values occur -> symbol codes and key geometry; entropy probe, repeat probe, gram keys (read-backs: the 256 presence flags, two duplicate counts, the number of grams in use)
    int geometry_and_probes()
    {
        int rc = SA_AMD_OK; (void)rc;
        // 1. sigma = 256 histogram -> symbol codes, bits per symbol, symbols per key
        HIP_TRY(hipMemsetAsync(w.hist, 0, 256 * 4, st));
        {
            int64_t blocks = ceil_div(ceil_div(n, 16), BH_THREADS);
            if (blocks > 2048) blocks = 2048;
            if (blocks < 1) blocks = 1;
            // (texts below the entropy probe's size: with counts, for the flat-histogram rule below)
            const bool counts = flat_rule_applies();
            if (counts) PROF(KC_BYTE_HIST, n, st, hipLaunchKernelGGL((k_byte_hist_counts), dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(BH_THREADS), 0, st, dT, n, w.hist));
            else PROF(KC_BYTE_HIST, n, st, hipLaunchKernelGGL((k_byte_hist), dim3((unsigned)blocks), dim3(BH_THREADS), 0, st, dT, n, w.hist));
        }
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
                flat_text = true;
            }
        }
        key_bits = make_key_params(hist, &P, &sigma, kb_max);      // (gram keys, step 2c, may shorten it)
        local.sigma = sigma; local.bits_per_symbol = P.bits; local.symbols_per_key = P.k;
        if (sigma == 1 && !tn.no_unary_shortcut) {
            // one byte value repeated: every suffix is a proper prefix of every longer one, the order is by length.  (The general
            // path gets there too -- 23 doubling rounds over one group of n members, 214 ms at 256 MiB -- and stays tested.)
            int64_t blocks = ceil_div(n, 256 * 16);
            if (blocks > 16384) blocks = 16384;
            PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_fill_descending), dim3((unsigned)blocks), dim3(256), 0, st, SA, n));
            unary_done = true;
            return SA_AMD_OK;
        }

        g_bits = bit_length((uint64_t)(n - 1 > 0 ? n - 1 : 1));
        bucket_top_bits = choose_bucket_bits();
        force_dense = tn.force_dense;
        text_ok = !force_dense && !tn.no_text_rounds;
        local_ok = !tn.no_local_sort;

        // 2. entropy probe: do the top 32 key bits already separate (almost) all suffixes?  Then the initial
        //    sort only needs those 4 digits and a cheap round on the low bits finishes the few ties.
        top_shift = 0;
        if (text_ok && local_ok && key_bits > 32 && !tn.no_top32) {
            bool use = tn.force_top32;
            if (!use && n >= tn.top32_probe_min_n) {
                // 2^20 samples, fewer for texts below 8 Mi suffixes (a power of two: the duplicate count hashes into 4 S slots)
                int64_t S = (int64_t)1 << 20;
                while (S > 1024 && S * 8 > n) S >>= 1;
                PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_sample_keys), dim3((unsigned)ceil_div(S, GK_THREADS)), dim3(GK_THREADS), 0, st, dT, P, n, S,
                                                        key_bits - 32, w.keysA));
                if ((rc = count_sample_dups(S, 8))) return rc;
                // the same samples, counted per bucket of the bucket sort: an estimate of its largest bucket (word 1 of the read-back)
                const int tb = choose_bucket_bits();
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
                        bucket_top_bits = 0;
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
        probe_dense = false;
        if (text_ok && local_ok && !top_shift && !force_dense && !tn.no_repeat_probe && n >= ((int64_t)1 << 24)) {
            const int64_t S = (int64_t)1 << 20;
            PROF(KC_MISC, S, st, hipLaunchKernelGGL((k_sample_repeat_keys), dim3((unsigned)ceil_div(S, GK_THREADS)), dim3(GK_THREADS), 0, st, dT, P, n, S,
                                                    w.keysA));
            if ((rc = count_sample_dups(S, 4))) return rc;
            uint32_t dups = 0;
            { const int rcw = read_words(&dups, w.total, 4, st); if (rcw) return rcw; }
            const double chance = (double)S * (double)S / 8589934592.0;           // 32-bit hash collisions among S samples
            const double frac = ((double)dups - chance) * (double)n / ((double)S * (double)S);
            probe_dense = frac > 0.04;
            if (trace) fprintf(stderr, "suffix_array_amd: repeat probe: %u duplicates among %lld samples (repeat index %.3f, threshold 0.04) -> %s\n",
                               dups, (long long)S, frac, probe_dense ? "rank doubling from the start" : "text-keyed rounds");
        }

        // 2c. gram keys (texts that did not take the 32-bit route): choose_gram_keys measures and decides; the probes above keep
        //     using the plain key
        if (!top_shift && !tn.no_gram_keys && n >= tn.gram_min_n && n >= 2 && sigma >= 2 && tn.key_bits_max == 64) {
            const int rcg = choose_gram_keys(dT, n, &P, &key_bits, w, st, tn, trace);
            if (rcg) return rcg;
            local.bits_per_symbol = P.bits; local.symbols_per_key = P.k;
        }

        return SA_AMD_OK;
    }

    // 4b. the 32-bit first stage: the top 32 key bits as (u32, u32) pairs -- two global passes + the in-LDS bucket sort, or four
    //     global passes (read-back: the largest bucket)
    int initial_sort_top32(uint32_t *vals0, uint8_t *packed_out, bool iota)
    {
        int rc = SA_AMD_OK; (void)rc;
        uint32_t *k32a = (uint32_t *)w.keysA, *k32b = (uint32_t *)w.keysB;
        // Two global passes over the top 16 key bits + one pass that orders every bucket (= value of those bits) in LDS, when an
        // average bucket fits a workgroup well (n = 2^28: 4096 pairs, 2^29: 8192); larger texts take two passes of NINE bits
        // (2^30: 2^18 buckets of 4096).  A text whose LARGEST bucket fits no workgroup -- known only once the two passes have
        // run -- builds its keys again and takes the four global passes.
        int top_bits = bucket_top_bits;      // 0: four global passes (choose_bucket_bits, the probe's estimate of the largest bucket)
        for (;;) {
            // the first radix pass's digit histogram comes out of k_build_keys (keys in registers there): one read of every key less
            const FirstCounts fc = sort_first_counts(w.ss, tn, n, true);
            const bool counted = n > 1;
            const int rbits = top_bits == 18 ? 9 : RADIX_BITS;
            // a text of all 256 byte values (code = byte, 8 symbols per key): the top 32 key bits are four text bytes -- the first
            // global pass reads them from the text (a quarter of the bytes) and no key array is built in front of it
            const bool text_route = top_bits != 0 && counted && iota && top_shift == 32 && onesweep_on(w.ss, tn) && tn.onesweep32_shape == 0 && !tn.no_text_keys;
            const bool text_keys = text_route && sigma == 256 && P.bits == 8 && packed_out == nullptr;
            // ... and with four symbols (DNA) the bit-packed text is the stream of keys: it is packed first (n / 4 bytes instead of a
            // key array of 4n), and counted and read by the first pass as it stands
            const bool packed_keys = text_route && sigma == 4 && P.bits == 2 && packed_out != nullptr;
            // Key bits for free: an index below 2^g_bits leaves 32 - g_bits bits of the value word unused, and the bucket sort stages
            // 16 bits per pair of which 32 - top_bits are low key bits.  When both have room (texts of 0.6 - 1 GiB: 18 top bits, 30-bit
            // indices) the first pass puts the two key bits BEHIND the 32 there and the bucket sort orders 34 bits: a quarter of the ties
            // on all 32 bits are left for its round on the low key bits (1 GiB of DNA: 22 % of the suffixes -> 6 %).
            int val_extra = 0;
            if ((text_keys || packed_keys) && !tn.no_value_bits) {
                val_extra = 32 - g_bits;
                if (val_extra > BK_MAX_LBITS - (32 - top_bits)) val_extra = BK_MAX_LBITS - (32 - top_bits);
                if (val_extra > 2) val_extra = 2;
                if (val_extra < 0) val_extra = 0;
            }
            if (counted) HIP_TRY(hipMemsetAsync(fc.zero_ptr, 0, fc.zero_bytes, st));
            if (text_keys || packed_keys) {
                int split = 2048 / fc.G;
                while (split > 1 && fc.chunk_elems / split < 16384) split /= 2;
                const int64_t sub = (ceil_div(fc.chunk_elems, split) + 15) & ~(int64_t)15;
                if (packed_keys) {
                    int64_t pblocks = ceil_div(ceil_div(n, 16), 256);
                    if (pblocks > 16384) pblocks = 16384;
                    PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_pack_text2), dim3((unsigned)pblocks), dim3(256), 0, st, dT, n, P, packed_out));
                    PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_packed2_upsweep32), dim3((unsigned)(fc.G * split)), dim3(SORT_THREADS), 0, st, (const uint8_t *)packed_out, n,
                                                                  fc.counts, 32 - top_bits, (1u << rbits) - 1u, fc.chunk_elems, fc.G, split, sub));
                } else
                PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_text_upsweep32), dim3((unsigned)(fc.G * split)), dim3(SORT_THREADS), 0, st, dT, n, fc.counts,
                                                              32 - top_bits, (1u << rbits) - 1u, fc.chunk_elems, fc.G, split, sub));
            } else
            PROF(KC_BUILD_KEYS, n, st, hipLaunchKernelGGL((k_build_keys<true>), dim3((unsigned)ceil_div(ceil_div(n, KB_TILE), KB_TPW)), dim3(KB_THREADS), 0, st, dT, n, P,
                                                          (uint64_t *)nullptr, vals0, k32a, top_shift, packed_out,
                                                          counted ? fc.counts : (uint32_t *)nullptr, fc.chunk_elems, fc.G, (1u << rbits) - 1u, top_bits ? 32 - top_bits : 0));
            SortResult<uint32_t> s32;
            SortJob<uint32_t> job{ k32a, w.valsA, k32b, w.valsB, n, top_bits ? 32 - top_bits : 0, 32 };
            job.iota = iota; job.first_counted = counted;
            if (top_bits) {
                job.rbits = rbits;
                job.text = text_keys ? dT : (packed_keys ? (const uint8_t *)packed_out : (const uint8_t *)nullptr);
                job.text_n = n; job.text_bits = packed_keys ? 2 : 8;
                job.val_extra = val_extra;
                rc = sort_pairs32(job, w.ss, st, tn, &s32, &local);
                if (rc) return rc;
                uint32_t *kout = (s32.keys == k32a) ? k32b : k32a;
                bool done = false, fused = false;
                uint32_t largest = 0;
                // the round on the low key bits of the suffixes tied on all 32 (first_round_from_sorted_keys) in the same launch
                const bool fuse = local_ok && !tn.no_fused_finish && !tn.no_bucket_finish && !timing_only();
                BucketFinish F = BucketFinish();
                KeySrc K = KeySrc();
                if (fuse) {
                    if ((rc = zero_finish_records())) return rc;
                    F.T = dT; F.n = n; F.cap = tn.group_cap; F.surv_bits = w.surv_bits; F.surv_head = w.isa; F.tile_cnt = w.tcnt; F.counters = w.total;
                    K.mode = KS_LOWKEY; K.kb = top_shift;
                }
                KeyParams Pf = P;
                Pf.packed = packed_out;             // (written by now: the fused round's text look-ups take the bit-packed text, a quarter of the lines)
                rc = bucket_sort32(s32.keys, s32.vals, kout, SA, n, top_bits, w.bk_start, w.ss.err + 2, st, tn, &done, &largest,
                                   fuse ? &F : nullptr, &Pf, &K, &fused, val_extra);
                if (rc) return rc;
                bucket_finished = done && fused;
                if (trace) fprintf(stderr, "suffix_array_amd: 32-bit first stage: %d global passes over the top %d key bits, largest bucket %u -> %s\n", s32.passes, top_bits, largest,
                                   done ? (fused ? "low bits and ties on all 32 ordered bucket by bucket in LDS" : "low bits ordered bucket by bucket in LDS")
                                        : "too large: keys rebuilt, four global passes");
                if (!done) { top_bits = 0; continue; }      // (nothing was launched: the finish buffers are zeroed again by whoever uses them)
                local.sort_passes += 1; local.sorted_elements += n;
                sorted32 = kout;
                sr.vals = SA; sr.passes = s32.passes + 1;
                sr.keys = (kout == k32a) ? w.keysA : w.keysB;
                break;
            }
            job.final_vals = SA;
            rc = sort_pairs32(job, w.ss, st, tn, &s32, &local);
            if (rc) return rc;
            sorted32 = s32.keys;
            sr.vals = s32.vals; sr.passes = s32.passes;
            sr.keys = (s32.keys == k32a) ? w.keysA : w.keysB;      // the 8n-byte buffer that now holds the sorted 32-bit keys
            break;
        }
        return SA_AMD_OK;
    }

    // 3-4. packed keys and the initial LSD sort, the last pass writing straight into SA
    int initial_sort()
    {
        int rc = SA_AMD_OK; (void)rc;
        // 3. packed keys, 4. initial sort: all key bits as (u64 key, u32 suffix) pairs, or only the top 32 bits as
        //    (u32, u32) pairs in 12 Ki-element tiles -- two thirds of the bytes per pass and half the passes
        sr.keys = w.keysA; sr.vals = w.valsA; sr.passes = 0;
        head_flags = nullptr;
        sorted32 = nullptr;               // top-32 stage: the sorted 32-bit keys (no 64-bit sorted array exists)
        bucket_finished = false;
        // value of pair i = i: not stored by k_build_keys, the first sort pass takes the index (saves 8 B / suffix)
        const bool iota = n >= 2 && key_bits > 0;
        uint32_t *vals0 = iota ? (uint32_t *)nullptr : w.valsA;
        // alphabets of 2, 4 or 16 symbols: k_build_keys also writes the text as bit-packed codes, which every later random
        // read of the text uses instead (a key becomes a bit field of two words; DNA shrinks to a quarter: cache-resident)
        uint8_t *packed_out = nullptr;
        if ((P.bits == 1 || P.bits == 2 || P.bits == 4) && n >= 64 && !tn.no_packed_text) {
            packed_out = w.packed;
            HIP_TRY(hipMemsetAsync(packed_out + (size_t)(n >> 3) * P.bits, 0, 64, st));     // the padding behind the last whole group
        }
        if (top_shift) {
            rc = initial_sort_top32(vals0, packed_out, iota);
            if (rc) return rc;
        } else {
            const FirstCounts fc = sort_first_counts(w.ss, tn, n, false);
            const bool counted = n > 1 && key_bits > 0;
            if (counted) HIP_TRY(hipMemsetAsync(fc.zero_ptr, 0, fc.zero_bytes, st));
            if ((rc = build_keys64(vals0, packed_out, fc, counted))) return rc;
            // (a text of ONE byte value -- a zero-filled file -- has the same key everywhere but at its end: its passes are the identity
            // and are looked for; any other text does not pay the read-backs)
            // diagnostic library, SA_AMD_SAMPLE_SORT=1 (a measured dead end, profiles/r04_sample_sort_64.txt): the sample sort -- two
            // distribution passes over quantile digits + every bucket ordered in LDS -- instead of one LSD pass per digit
            bool ss_done = false;
#ifdef SA_AMD_DIAG
            if (iota && counted && tn.sample_sort && n >= tn.sample_sort_min_n && key_bits > 32 && onesweep_on(w.ss, tn) && !timing_only()) {
                const size_t need_big = ((size_t)ceil_div(n, SS_TILE) + SS_WAYS) * SS_IDS2 * 4;
                if (need_big <= (size_t)n * 4 && (size_t)n * 4 >= ((size_t)4 << 20)) {
                    rc = sample_sort64(w.keysA, w.keysB, w.keysC, w.valsA, w.valsB, w.U0, w.U1, w.isa, w.G0, w.bk_start, SA, n, key_bits, w.ss, st, &local, tn,
                                       &ss_done, trace);
                    if (rc) return rc;
                    if (ss_done) { sr.keys = w.keysB; sr.vals = SA; sr.passes = 3; sr.skipped = 0; }
                    else {
                        // (cannot sort this text in workgroup-sized buckets: the keys again, then the LSD engine)
                        HIP_TRY(hipMemsetAsync(fc.zero_ptr, 0, fc.zero_bytes, st));
                        if ((rc = build_keys64(vals0, packed_out, fc, true))) return rc;
                    }
                }
            }
#endif
            if (!ss_done) {
            // Group-start flags instead of sorted keys from the last pass (head_flags above): asked for when the dense route is
            // expected -- its first re-rank is the only reader of the sorted keys then.  Tuning::head_flags 0: never, 2: always
            // (the routes that need the keys rebuild them: rebuild_sorted_keys); diagnostic library only.
            const bool dense_expected = force_dense || probe_dense || !text_ok;
            const bool want_flags = tn.head_flags != 0 && (tn.head_flags == 2 || dense_expected) && flags_slab_ok && onesweep_on(w.ss, tn) && !timing_only() &&
                                    !tn.fused64 && n >= 2 && key_bits > 0;
            SortJob<uint64_t> job{ w.keysA, w.valsA, w.keysB, w.valsB, n, 0, key_bits };
            job.final_vals = SA;
            job.iota = iota; job.may_skip = sigma == 1; job.first_counted = counted;
            job.head_flags = want_flags ? (uint8_t *)w.keysC : (uint8_t *)nullptr;
            rc = sort_pairs(job, w.ss, st, tn, &sr, &local);
            if (rc) return rc;
            if (want_flags && sr.passes > 0 && sr.vals == SA) head_flags = (uint8_t *)w.keysC;      // (the last pass always runs: it delivers into SA)
            if (trace && head_flags) fprintf(stderr, "suffix_array_amd: initial sort: the last pass wrote group-start flags, not the sorted keys\n");
            }
        }
        P.packed = packed_out;
        if (sr.vals != SA) {   // n == 1: no pass ran, the values are still in the input buffer
            PROF(KC_MISC, n, st, hipLaunchKernelGGL((k_copy_u32), dim3(1), dim3(256), 0, st, sr.vals, SA, n));
        }

        return SA_AMD_OK;
    }

    // list buffers; the fast finish of the 32-bit first stage / the opt-in fused first text round (read-backs: tied counts)
    int first_round_from_sorted_keys()
    {
        int rc = SA_AMD_OK; (void)rc;
        // 4. group heads of the initial order; how many suffixes are still tied with a neighbour
        L.U = w.U0; L.Un = w.U1; L.G = w.G0; L.Gn = w.G1;
        L.V = w.valsA;
        tiles = ceil_div(n, RR_TILE);
        m32 = 0;
        L.m = 0;
        L.rkA = w.keysA; L.rkB = w.keysB;          // key buffers of the refinement rounds
        sorted0 = sr.keys;                      // the initial keys in SA order (kept for the rank look-ups)
        lists_ready = false;                         // (L.U, L.G, L.V) already hold the tied suffixes
        depth = P.k;                               // symbols the current order is sorted by
        // Text-keyed rounds pack their symbols as bit fields of ceil(log2 sigma) bits whatever the alphabet: a secondary key only
        // has to preserve the order inside one round, and the base-sigma form costs a 64-bit multiply per symbol in kernels
        // that are instruction-bound (k_group_sort: 26 ps per suffix however small the text).  English-like sigma = 56: six
        // symbols in 36 bits either way.
        Ptext = P;
        if (P.bits == 0) Ptext.bits = bit_length(P.sigma - 1);
        Ptext.gram = 0;                                    // (gram ranks are the initial keys' business only)
        s_sym = 0; tkb = 0;                            // symbols per round, bits of their packed key
        {
            const int room = 64 - g_bits;                   // bits left below the group head
            s_sym = room / Ptext.bits;
            if (s_sym > 64) s_sym = 64;
            tkb = s_sym * Ptext.bits;
        }
        finished32 = false; fused64 = false;
        if (top_shift && local_ok && !tn.no_fused_finish && !timing_only()) {
            // fast finish of the 32-bit first stage: one pass orders every small group by its low key bits in place
            // (k_finish_sorted); only if some group is too large for it does the general path below run instead
            const int cap = tn.group_cap;
            uint32_t *surv_bits = w.surv_bits, *surv_head = w.isa;  // (the ISA is not in use before the doubling rounds)
            if (!bucket_finished) {      // (else k_bucket_sort has done this round while it had the buckets in LDS, into the same records)
            if ((rc = zero_finish_records())) return rc;
            KeySrc K = KeySrc(); K.mode = KS_LOWKEY; K.kb = top_shift;
            PROF(KC_FINISH, n, st, hipLaunchKernelGGL((k_finish_sorted<uint32_t, KS_LOWKEY, false>), dim3((unsigned)ceil_div(n, FT_TILE)), dim3(FT_THREADS),
                                                     0, st, sorted32, SA, dT, P, n, K, cap, surv_bits, surv_head, w.tcnt, w.total, (uint32_t *)nullptr,
                                                     (uint32_t *)nullptr, (uint32_t *)nullptr));
            }
            // (k_bucket_sort counts its survivors itself: the scan of the tiles' counts runs only if there are any)
            if (!bucket_finished) PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total));
            uint32_t cnt3[3] = { 0, 0, 0 };                       // still tied on 64 bits, members of groups nobody owned, tied on 32 bits
            {
                uint32_t words[64 + RR_CHG_COUNTERS * 32];         // (the tied-slot counts are spread over w.chg, directly behind w.total)
                const int rcw = read_words(words, w.total, sizeof(words), st); if (rcw) return rcw;
                cnt3[0] = words[0]; cnt3[1] = words[1];
                for (int c = 0; c < RR_CHG_COUNTERS; ++c) cnt3[2] += words[64 + c * 32];
                if (bucket_finished) {
                    cnt3[0] = 0;
                    for (int c = 0; c < RR_CHG_COUNTERS; ++c) cnt3[0] += words[64 + c * 32 + 1];
                    if (cnt3[0] != 0 && cnt3[1] == 0)
                        PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total));
                }
            }
            if (cnt3[1] == 0) {
                finished32 = true;
                L.m = cnt3[0];
                local.locally_sorted += cnt3[2];
                local.unresolved_after_initial = L.m;
                if (L.m > 0) {
                    PROF(KC_RR_APPLY, n, st, hipLaunchKernelGGL((k_surv_compact), dim3((unsigned)tiles), dim3(256), 0, st, (const uint32_t *)surv_bits,
                                                                (const uint32_t *)surv_head, (const uint32_t *)SA, n, (const uint32_t *)w.tcnt,
                                                                (const uint32_t *)w.total, L.U, L.G, L.V));
                    L.keys_beside(w, sr.keys);
                    lists_ready = true;
                }
            }
        }
        // (SA_AMD_SPARSE_DIV moves the text-round / doubling boundary for the tests: then the general route decides, as before)
        // Opt-in (SA_AMD_FUSED64=1): measured on C3 the one-pass round costs 8.2 ms against the 4.3 ms of k_group_sort on the tied
        // list -- with 68 % of the slots tied the work list is six entries per thread -- and the whole build 31.0 instead of 28.8 ms.
        if (!top_shift && text_ok && local_ok && s_sym > 0 && tn.fused64 && !tn.no_fused_finish && !tn.sparse_div_set && !timing_only()) {
            // the first text-keyed round straight from the sorted keys (k_finish_sorted): groups of up to `cap` members are
            // ordered in place by the next s_sym symbols, their still-tied members recorded by slot; the members of larger
            // groups are listed (k_todo_compact) and take the general route (refine_list + re-rank), joining the same record;
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
            KeySrc K = KeySrc(); K.mode = KS_TEXT; K.h = depth; K.s = s_sym; K.kb = tkb;
            PROF(KC_FINISH, n, st, hipLaunchKernelGGL((k_finish_sorted<uint64_t, KS_TEXT, true>), dim3((unsigned)ft_tiles), dim3(FT_THREADS), 0, st,
                                                     (const uint64_t *)sorted0, SA, dT, Ptext, n, K, cap, w.surv_bits, surv_head, w.surv_cnt, w.total,
                                                     w.todo_bits, w.ft_cnt, w.ft_head));
            PROF(KC_RR_SCAN, ft_tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.ft_cnt, w.ft_head, ft_tiles, w.total + 3));
            uint32_t cnt4[4] = { 0, 0, 0, 0 };                    // [2] tied after the initial sort, [3] members left to the general route
            {
                uint32_t words[64 + RR_CHG_COUNTERS * 32];
                const int rcw = read_words(words, w.total, sizeof(words), st); if (rcw) return rcw;
                cnt4[0] = words[0]; cnt4[1] = words[1]; cnt4[3] = words[3];
                for (int c = 0; c < RR_CHG_COUNTERS; ++c) cnt4[2] += words[64 + c * 32];
            }
            local.unresolved_after_initial = cnt4[2];
            const int64_t m_todo = cnt4[3];
            local.locally_sorted += (int64_t)cnt4[2] - m_todo;
            L.keys_beside(w, sr.keys);
            if (m_todo > 0) {
                PROF(KC_RR_APPLY, n, st, hipLaunchKernelGGL((k_todo_compact<uint64_t>), dim3((unsigned)ft_tiles), dim3(FT_THREADS), 0, st,
                                                            (const uint64_t *)sorted0, (const uint32_t *)SA, n, (const uint32_t *)w.todo_bits,
                                                            (const uint32_t *)w.ft_cnt, (const uint32_t *)w.ft_head, (const uint32_t *)(w.total + 3),
                                                            L.U, L.G, L.V));
                L.m = m_todo;
                Refined rf;
                bool big_local = true;                             // (large groups: the global sort does the work either way)
                if ((rc = refine_list(Ptext, K, &big_local, &rf))) return rc;
                if ((rc = rr_count<false>(rf.keys, L.U, L.m, nullptr, 0, nullptr, w.ft_cnt, w.ft_head))) return rc;
                if ((rc = rr_scan(L.m, w.ft_cnt, w.ft_head, w.total + 4))) return rc;
                RrApply a = round_args(rf);
                a.tile_cnt = w.ft_cnt; a.tile_head = w.ft_head; a.tile_total = w.total + 4;
                a.has_isa = w.surv_bits; a.pair_v = w.surv_cnt;
                if ((rc = rr_apply<false, true, 4>(rf.keys, a))) return rc;
            }
            PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.surv_cnt, w.thead, tiles, w.total));
            { const int rcw = read_words(&m32, w.total, 4, st); if (rcw) return rcw; }
            L.m = m32;
            L.U = w.U0; L.G = w.G0; L.V = w.valsA; L.Un = w.U1; L.Gn = w.G1;
            if (L.m > 0)
                PROF(KC_RR_APPLY, n, st, hipLaunchKernelGGL((k_surv_compact), dim3((unsigned)tiles), dim3(256), 0, st, (const uint32_t *)w.surv_bits,
                                                            (const uint32_t *)surv_head, (const uint32_t *)SA, n, (const uint32_t *)w.surv_cnt,
                                                            (const uint32_t *)w.total, L.U, L.G, L.V));
            fused64 = true;
            lists_ready = true;
            depth += s_sym;
            local.text_rounds++;
            local.rounds++;
            if (trace) fprintf(stderr, "suffix_array_amd: text round %d depth %lld: tied %lld -> %lld  (%.2f ms)\n", local.text_rounds, (long long)depth, (long long)cnt4[2], (long long)L.m, lap());
        }
        return SA_AMD_OK;
    }

    // 4. group heads of the initial order: how many suffixes are still tied (read-back: that count)
    int group_heads()
    {
        int rc = SA_AMD_OK; (void)rc;
        if (!finished32 && !fused64) {
        // (64-bit keys: also every tile's first group start: the dense route's first ranks are tail ranks, k_rr_apply FTAIL)
        rc = top_shift ? rr_count<true, uint32_t>(sorted32, nullptr, n)
           : head_flags ? rr_count<true, uint64_t, true, true>((const uint64_t *)sr.keys, nullptr, n, w.tnext)
                        : rr_count<true, uint64_t, true>((const uint64_t *)sr.keys, nullptr, n, w.tnext);
        if (rc) return rc;
        if ((rc = rr_scan(n))) return rc;
        { const int rcw = read_words(&m32, w.total, 4, st); if (rcw) return rcw; }
        L.m = m32;
        local.unresolved_after_initial = L.m;
        if (timing_only()) L.m = 0;   // diag library: ablation kernels produce wrong orders; stop here
        }
        return SA_AMD_OK;
    }

    // the suffixes tied on the top 32 key bits are ordered by their low key bits (read-back: tied on all 64 bits)
    int finish_top32_ties()
    {
        int rc = SA_AMD_OK; (void)rc;
        if (!finished32 && top_shift && L.m > 0) {
            // finish the initial sort: the suffixes tied on the top 32 bits are ordered by their low key bits
            L.keys_beside(w, sr.keys);
            if ((rc = rr_apply<true, false, 1, uint32_t>(sorted32, first_args(0u, w.has_isa)))) return rc;
            Refined rf;
            KeySrc K = KeySrc(); K.mode = KS_LOWKEY; K.kb = top_shift;
            if ((rc = refine_list(P, K, &local_ok, &rf))) return rc;
            if ((rc = rr_count<false>(rf.keys, L.U, L.m))) return rc;
            if ((rc = rr_scan(L.m))) return rc;
            if ((rc = rr_apply<false, true, 3>(rf.keys, round_args(rf)))) return rc;
            { const int rcw = read_words(&m32, w.total, 4, st); if (rcw) return rcw; }
            L.m = m32;
            L.advance(rf);
            lists_ready = true;
            local.unresolved_after_initial = L.m;           // now: tied on the whole 64-bit key, as after a full sort
        }
        return SA_AMD_OK;
    }

    // 5. dense route: ranks + ISA; otherwise compaction and the text-keyed rounds (read-back per round: tied count)
    int rank_setup_and_text_rounds()
    {
        int rc = SA_AMD_OK; (void)rc;
        // 5. refinement of the tied suffixes.  Three regimes:
        //   text rounds  while more than n / SPARSE_DIV suffixes are tied: secondary key = the next symbols of
        //                the text itself (no rank array needed yet), depth grows by s symbols per round;
        //   sparse       few tied suffixes: prefix doubling, ranks looked up without an ISA (sparse_key2);
        //   dense        prefix doubling with a full ISA (repetitive texts, or forced for A/B measurements).
        key2_bits = bit_length((uint64_t)(2 * n));
        const int64_t sparse_div = tn.sparse_div;      // (SA_AMD_SPARSE_DIV moves the boundary for tests / A-B)
        const int64_t sparse_limit = n / sparse_div;
        sparse = false;
        const bool dense_first = L.m > 0 && !lists_ready && (force_dense || (!text_ok && L.m > sparse_limit) || (probe_dense && L.m > sparse_limit));
        if (L.m > 0 && dense_first) {
            // ranks (ISA scatter) + compaction of the tied suffixes; SA already holds the sorted order
            // the first ranks are TAIL ranks (a group's last slot + 1), the form the dense rounds keep (k_rr_apply): the first doubling
            // round then writes only the ranks that change (SA_AMD_NO_FIRST_TAIL=1: head ranks, everything rewritten in round 1)
            isa_tail_ranks = !tn.no_first_tail;
            if (isa_tail_ranks)
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
                if ((rc = rr_apply_setup<2>(a))) return rc;
                if (from_sa) {
                    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, dSA, (uint32_t)n);
                    LAUNCH_CHECK(st);
                    rc = scatter_binned(w.ss, w.isa, dSA, pk32 + H, sk32, sk32 + H, n + 1, n, st, &local, tn, false, pk32);
                } else
                    rc = scatter_binned(w.ss, w.isa, (uint32_t *)pk, w.U1, (uint32_t *)sr.keys, w.G1, n, n, st, &local, tn);
                if (rc) return rc;
            } else if ((rc = rr_apply_setup<0>(a))) return rc;
        } else if (L.m > 0) {
            // compaction only; the sorted initial keys stay intact for the rank look-ups
            if ((rc = rebuild_sorted_keys())) return rc;
            HIP_TRY(hipMemsetAsync(w.has_isa, 0, ((size_t)n + 31) / 32 * 4, st));
            if (!lists_ready) {
                L.keys_beside(w, sr.keys);
                if ((rc = rr_apply<true, false, 1>((const uint64_t *)sorted0, first_args(0u, w.has_isa)))) return rc;
            }
            // ---- text-keyed rounds ----
            bool progressing = true;     // a text round that resolves little (runs, long repeats) is the last one

            bool counters_clear = false;      // (RoundCtl: one read-back per round while the rounds have nothing for the global sort)
            while (text_ok && s_sym > 0 && L.m > sparse_limit && local.text_rounds < tn.max_text_rounds && progressing) {
                if ((rc = early_maybe_start())) return rc;
                const int64_t m_before = L.m;
                Refined rf;
                KeySrc K = KeySrc(); K.mode = KS_TEXT; K.h = depth; K.s = s_sym; K.kb = tkb;
                RoundCtl ctl;
                ctl.defer = prev_clean && local_ok && !tn.no_defer;
                ctl.counters_clear = counters_clear;
                if ((rc = refine_list(Ptext, K, &local_ok, &rf, false, nullptr, &ctl))) return rc;
                uint32_t words[RC_WORDS];
                if ((rc = finish_round<3, false>(Ptext, K, ctl, rf, RrApply(), words, sizeof(words), false, nullptr))) return rc;
                prev_clean = ctl.m_flagged == 0;
                counters_clear = true;
                L.m = words[0];
                L.advance(rf);
                depth += s_sym;
                local.text_rounds++;
                local.rounds++;
                progressing = L.m * 4 <= m_before * 3;
                if (trace) fprintf(stderr, "suffix_array_amd: text round %d depth %lld: tied %lld -> %lld  (%.2f ms)\n", local.text_rounds, (long long)depth, (long long)m_before, (long long)L.m, lap());
            }
            if (L.m > sparse_limit) {
                // still many ties (repetitive text): build the ISA of the current order and double densely
                int64_t blocks = ceil_div(n, 256);
                if (blocks > 16384) blocks = 16384;
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
                    PROF(KC_SCATTER, n, st, hipLaunchKernelGGL((k_isa_from_sa), dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t *)SA, w.isa, n));
                blocks = ceil_div(L.m, 256);
                if (blocks > 16384) blocks = 16384;
                PROF(KC_SCATTER, L.m, st, hipLaunchKernelGGL((k_isa_tied), dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t *)L.V,
                                                           (const uint32_t *)L.G, w.isa, L.m, n));
            } else {
                sparse = L.m > 0;
            }
        }
        local.sparse_mode = sparse ? 1 : 0;
        if (trace) fprintf(stderr, "suffix_array_amd: initial sort + text rounds + rank set-up done, %lld tied (%.2f ms since the last line)\n", (long long)L.m, lap());

        return SA_AMD_OK;
    }

    // prefix doubling on what is still tied, dense (ISA) or sparse (read-backs per round: tied count, ranks written)
    int doubling_rounds()
    {
        int rc = SA_AMD_OK; (void)rc;
        // prefix doubling on what is still tied; `depth` symbols are sorted, so the first offset is `depth`
        const int64_t depth_text = depth;
        int64_t h = depth;
        bool chase_ok = false;
        int split_rest = 0;                               // rounds the three-way split sits out (refine_list)
        bool parent_tail = isa_tail_ranks;                // the ranks in the ISA are tail ranks (set by the first dense round, or by the rank set-up of the dense route)
        int64_t changed_prev = isa_tail_ranks ? L.m : 0;    // ranks the last dense round wrote (none yet: expect every rank to change)
        int64_t m_local_off = L.m;                          // size of the tied list when the local pass was last in use
        int rounds_local_off = 0;
        // read-backs (RoundCtl): a round whose predecessor had nothing for the global sort defers that question and blocks ONCE
        bool all_small = false;                           // ... and listed no group for k_group_sort_big: no group is larger than GS_CAP any more
        bool counters_clear = false;                      // the previous round's k_rr_scan_round zeroed the big-group counters
        // dense rounds write a slot of SA once, in the round its suffix leaves the tied list (k_rr_apply sa_final); the loop runs
        // until the list is empty, so every slot gets its final value.  Sparse rounds look suffixes up in SA (sparse_key2): every round
        const int sa_final = (!sparse && !tn.sa_every_round) ? 1 : 0;
        while (L.m > 0) {
            if (local.rounds >= 48) return SA_AMD_EINTERNAL;
            if ((rc = early_maybe_start())) return rc;     // (every slot outside the tied list is final from here on)
            // the same refinement machinery as the text rounds, keyed by ranks -- small groups (a long repeat gives millions of
            // pairs) are ordered in LDS, only large groups go through the global sort.  Dense: ranks from the ISA; sparse:
            // looked up without one (sparse_key2)
            KeySrc K = KeySrc();
            K.mode = sparse ? KS_SPARSE : KS_RANK; K.h = h; K.kb = key2_bits; K.isa = w.isa;
            // dense rounds chase (up to `chase` rank look-ups per member inside one launch) once a round has had no group left
            // for the global sort: from then on every surviving group is known to share (iters + 1) * h symbols
            // the local pass was given up because (nearly) every member sat in a group no tile can own: it is tried again when the
            // list has halved, and every third round -- if refine_list then finds the average group small enough for a tile (large
            // lists count their groups anyway; a Fibonacci word's groups shrink while the list does not, a periodic text's never do)
            if (!local_ok && !tn.no_local_sort && L.m * 2 < m_local_off) local_ok = true;
            const bool retry_local = !local_ok && ++rounds_local_off >= 3;
            K.iters = (!sparse && local_ok && chase_ok) ? (L.m >= tn.chase_big_min ? tn.chase_big : tn.chase) : 1;
            if (K.iters > 1) K.mode = KS_CHASE;
            K.has_isa = w.has_isa; K.sorted_keys = sorted0; K.sorted_top32 = sorted32; K.sa = SA; K.depth = depth_text; K.top_shift = top_shift;
            Refined rf;
            if (local_ok) { m_local_off = L.m; rounds_local_off = 0; }
            // binned or direct ISA stores: by the number of ranks this round is expected to write -- all of them when the parents'
            // ranks are not tail ranks yet, otherwise about as many as the round before wrote
            const int64_t expect = (!parent_tail || L.m < changed_prev) ? L.m : changed_prev;
            const bool bin = !sparse && binned(n, expect, tn);
            RoundCtl ctl;
            ctl.defer = prev_clean && !bin && local_ok && !tn.no_defer;
            ctl.skip_big = all_small;
            ctl.counters_clear = counters_clear;
            if ((rc = refine_list(P, K, &local_ok, &rf, retry_local, &split_rest, &ctl))) return rc;
            if (retry_local && rf.m_global < L.m) { m_local_off = L.m; rounds_local_off = 0; }      // (the local pass ran again; such a round is never deferred)
            // w.total (64 words) and, dense rounds, the changed-rank counters behind it (w.chg) in one read-back
            uint32_t words[64 + RR_CHG_COUNTERS * 32];
            RrApply a;
            a.g_shift = key2_bits;
            if (sparse) a.has_isa = w.has_isa;
            else { a.tile_next = w.tnext; a.parent_tail = parent_tail ? 1 : 0; a.changed_cnt = w.chg; a.sa_final = sa_final; }
            // a binned round: L.G has been consumed by the gather, the other key buffer by nothing -- they take the (suffix, rank) pairs
            if (bin) { a.pair_k = (rf.keys == L.rkA) ? L.rkB : L.rkA; a.pair_v = L.G; }
            const size_t wb = sparse ? (size_t)RC_WORDS * 4 : sizeof(words);
            rc = sparse ? finish_round<1, false>(P, K, ctl, rf, a, words, wb, retry_local, &split_rest)
                 : bin  ? finish_round<2, true>(P, K, ctl, rf, a, words, wb, retry_local, &split_rest)
                        : finish_round<0, true>(P, K, ctl, rf, a, words, wb, retry_local, &split_rest);
            if (rc) return rc;
            if (ctl.missed) ++deferred_misses;
            prev_clean = ctl.m_flagged == 0;
            if (prev_clean && (ctl.big_listed == 0 || L.m <= GS_CAP)) all_small = true;
            counters_clear = true;                        // (k_rr_scan_round ran ungated in the end)
            {
                m32 = words[0];
                if (!sparse) {
                    changed_prev = 0;
                    for (int c = 0; c < RR_CHG_COUNTERS; ++c) changed_prev += words[64 + c * 32];
                    parent_tail = true;
                }
            }
            if (trace) fprintf(stderr, "suffix_array_amd: doubling round %d h %lld (%s, %d look-ups, %lld through the global sort): tied %lld -> %u, %lld ranks written\n", local.rounds + 1, (long long)h, sparse ? "sparse" : "dense", K.iters, (long long)rf.m_global, (long long)L.m, m32, sparse ? -1ll : (long long)changed_prev), fprintf(stderr, "    (%.2f ms)\n", lap());
            if (trace && !sparse) fprintf(stderr, "    (group starts read from %s)\n", rf.status ? "status bytes" : "keys");
            L.m = m32;
            L.advance(rf);
            // every group that is still tied went through K.iters look-ups -- unless some went through the global sort (one look-up)
            h *= (K.iters > 1 && rf.m_global == 0) ? (int64_t)(K.iters + 1) : 2;
            chase_ok = rf.m_global == 0;
            local.rounds++;
        }
        return SA_AMD_OK;
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
    if ((rc = B.geometry_and_probes())) return rc;
    if (!B.unary_done) {
    if ((rc = B.initial_sort())) return rc;
    if ((rc = B.first_round_from_sorted_keys())) return rc;
    if ((rc = B.group_heads())) return rc;
    if ((rc = B.finish_top32_ties())) return rc;
    if ((rc = B.rank_setup_and_text_rounds())) return rc;
    if ((rc = B.doubling_rounds())) return rc;
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
    if (B.trace) fprintf(stderr, "suffix_array_amd: %d blocking read-backs in this build (%d rounds deferred their mid-round count and had to run the global sort after all)\n", g_readbacks, B.deferred_misses);
    g_prof.resolve();
    g_last_stats = local;
    if (stats) *stats = local;
    return SA_AMD_OK;
}

}  // namespace sa
