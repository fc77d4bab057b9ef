// host/refine_round.hpp -- one refinement round of the tied list (RefineRound), what it works on (BuildCore) and what the rounds
// hand on (RoundState); DESIGN.md section 2.  Not a header to include on its own: host/pipeline.hpp includes it once, behind
// Workspace and scatter_binned and its own includes (Tuning, sort_pairs, read_words, PROF, the kernels).  The loops are there.
#pragma once
#include <type_traits>

namespace sa {

struct Refined {
    const uint64_t *keys; const uint32_t *vals; uint32_t *vnext;
    int64_t m_global;                      // members ordered by the global sort
    const uint8_t *status = nullptr;       // != nullptr: the round's status bytes (RS_*, kernels/common.hpp) -- the re-rank reads the group starts from them, `keys` holds true keys at RS_KEYED places only
};

// Read-backs of a refinement round (RefineRound::run; DESIGN.md section 2, Read-backs): a DEFERRED round leaves the count of the
// members its local pass could not order on the device (w.total[RC_FLAGGED]), launches the re-rank kernels GATED on it -- they do
// nothing when it is not zero -- and reads everything once at its end.  The words of that read-back: w.total (TOTAL_WORDS
// words) and, directly behind it, the spread counters w.chg.
constexpr int TOTAL_WORDS = 64, ROUND_WORDS = TOTAL_WORDS + RR_CHG_COUNTERS * 32;
constexpr int RC_TIED = 0;             // members still tied behind the re-rank (the total of its scan)
constexpr int RC_FLAGGED = 16, RC_GROUPS = 8, RC_BIG_LISTED = 12, RC_BIG_ORDERED = 13, RC_WORDS = 17;      // words of w.total (RC_GROUPS: flagged groups behind a local pass, all groups of the list from count_groups -- the same word)
constexpr int RC_BIG_LISTED_SAVED = 14, RC_BIG_ORDERED_SAVED = 15;     // ... where k_rr_scan_round puts the two big-group counters before it zeroes them for the next round
constexpr int RC_BIG_CLASS = 17;       // ... and [17], [18]: the lengths of the two lists k_big_classify sorts the listed heads into; zeroed with the two counters
static_assert(RC_BIG_CLASS == RC_BIG_LISTED + RR_CLEAR_CLASS && RC_BIG_CLASS + 2 <= TOTAL_WORDS, "k_rr_scan_round zeroes them relative to the big-group counters; w.total has 64 words");
// w.chg as read back behind w.total: counter `which` summed over its RR_CHG_COUNTERS words, 32 words apart (0: ranks a dense
// round changed, slots tied on 32 bits behind k_finish_sorted; 1: slots still tied behind k_bucket_sort's fused finish)
static inline int64_t chg_sum(const uint32_t *words, int which = 0)
{ int64_t s = 0; for (int c = 0; c < RR_CHG_COUNTERS; ++c) s += words[TOTAL_WORDS + c * 32 + which]; return s; }

// What one round leaves for the next (DeviceBuild::rs, RefineRound::S); the doubling rounds set their part when they start.
struct RoundState {
    bool prev_clean = true;             // the last refinement round's local pass ordered every member (optimistic for the first one: a miss costs three empty launches)
    bool counters_clear = false;        // the previous round's k_rr_scan_round zeroed the big-group counters (w.total[RC_BIG_LISTED .. +1])
    bool all_small = false;             // ... and listed no group for k_group_sort_big: no group is larger than GS_CAP any more, it is not launched
    bool local_ok = false;              // the local pass is in use (RefineRound::use_local switches it)
    int64_t m_local_off = 0;            // size of the tied list when the local pass was last in use
    int rounds_local_off = 0;           // rounds since then
    bool chase_ok = false;              // the last dense round left no group to the global sort: the next one chases
    int split_rest = 0;                 // rounds the three-way split sits out after its count pass found no majority (doubling rounds only)
    bool parent_tail = false;           // the ranks in the ISA are tail ranks (set by the first dense round, or by the rank set-up of the dense route)
    int64_t changed_prev = 0;           // ranks the last dense round wrote (none yet: expect every rank to change)
    int deferred_misses = 0;            // rounds that deferred their mid-round read-back and did have members for the global sort 
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

// The arguments of k_rr_apply (kernels/rerank.hpp) by name, each defaulting to "not used"; BuildCore::rr_apply launches it.
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

// f(std::integral_constant<int, M>) for the M among Ms that equals a round's KeySrc::mode, for ELSE when none does
template <int ELSE, int... Ms, class F>
static inline int by_mode(int mode, F &&f)
{
    int rc = SA_AMD_OK;
    const bool hit = ((mode == Ms ? (rc = f(std::integral_constant<int, Ms>()), true) : false) || ...);
    return hit ? rc : f(std::integral_constant<int, ELSE>());
}

// The part of a device build (DeviceBuild, host/pipeline.hpp) that the refinement rounds work on.
struct BuildCore {
    const uint8_t *dT;                  // ---- inputs ----
    uint32_t *dSA, *SA;                 // SA = dSA + 1: the n sorted suffixes behind the sentinel slot
    int64_t n;
    hipStream_t st;
    Tuning tn;
    Workspace w;
    sa_amd_stats local;
    int g_bits = 0, key2_bits = 0;      // bits of a slot, of a doubling round's secondary key
    bool flags_slab_ok = true;          // w.keysC is device memory (reduced-memory route: it may be the pinned host block -- then the key route is taken)
    TiedList L;

    // ---- the re-rank step: k_rr_count, k_rr_scan (a round: k_rr_scan_round, RefineRound::rerank), k_rr_apply (kernels/rerank.hpp) ----
    // One launcher each, over the RR_TILE-element tiles of m elements; tile_cnt / tile_head / total == nullptr: the workspace's.
    // FLAGS: the groups come from `status` (the first re-rank behind a flags pass of the initial sort: InitialOrder::head_flags; a round: its status bytes), not from the keys
    template <bool FIRST, typename KeyT = uint64_t, bool PARENTS = false, bool FLAGS = false>
    int rr_count(const KeyT *keys, const uint32_t *U, int64_t m, uint32_t *tile_first = nullptr, int g_shift = 0, const uint32_t *gate = nullptr,
                 uint32_t *tile_cnt = nullptr, uint32_t *tile_head = nullptr, const uint8_t *status = nullptr)
    {
        PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_rr_count<FIRST, KeyT, PARENTS, FLAGS>), dim3(rr_count_grid<FLAGS>(m)), dim3(RR_THREADS), 0, st, keys, U, m,
                                                    tile_cnt ? tile_cnt : w.tcnt, tile_head ? tile_head : w.thead, 0, tile_first, g_shift, gate,
                                                    FLAGS ? status : (const uint8_t *)nullptr));
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
                                                      FLAGS ? a.status : (const uint8_t *)nullptr));
        return SA_AMD_OK;
    }
    // what every re-rank of the tied list shares: the refined order in, the next list out
    RrApply round_args(const Refined &rf, RrApply a = RrApply()) const
    {
        a.V = rf.vals; a.U = L.U; a.m = L.m; a.SA = SA; a.ISA = w.isa; a.Uo = L.Un; a.Go = L.Gn; a.Vo = rf.vnext; a.n_text = (uint32_t)n;
        return a;
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

    // Where a dense doubling round keeps its status bytes (RS_*, kernels/common.hpp; nullptr: the round takes the key route): in
    // w.keysC, one byte per member -- not in L.Gn, where k_rr_apply writes the next list's group heads while it reads them.  On
    // the route that doubles straight from the initial order w.keysC is dead by then (its group-start flags are consumed by the
    // rank set-up, early_finish takes it when the rounds are over); behind text rounds it is a key buffer of the rounds
    // (keys_beside) and on the reduced-memory route it may be pinned host memory (flags_slab_ok): keys then.
    uint8_t *round_status_slab(const KeySrc &K) const
    {
        if (tn.round_flags == 0 || (K.mode != KS_RANK && K.mode != KS_CHASE)) return nullptr;
        if (!flags_slab_ok || L.rkA == w.keysC || L.rkB == w.keysC) return nullptr;
        return (uint8_t *)w.keysC;
    }
};

// One refinement round of the tied list with a secondary key taken from the text or the ranks (KeySrc): afterwards every
// group is ordered by (group head << kb) | key2 and re-ranked.  Small groups: gather fused with the in-LDS group sort
// (k_group_sort); groups no tile owns, or everything when use_local is off: plain gather + global radix sort.  Made once per round:
// its members are what the steps share, each step does one thing, run() is the sequence.  L.Un / L.Gn: free until the re-rank.
constexpr int NO_RERANK = -1;              // run<NO_RERANK>: stop in front of the re-rank (the caller re-ranks the order in rf itself)
struct RefineRound {
    BuildCore &B;
    const KeyParams &Pk;
    KeySrc K;
    RoundState &S;                         // read: all_small, counters_clear, parent_tail; written: local_ok, split_rest
    const bool defer;                      // do not read the local pass's counts back: re-rank gated, one read-back (asked for only while the local pass is on)
    const bool doubling, retry_local;      // a doubling round: the split may sit rounds out (S.split_rest); its local pass is off: see whether the groups have become small enough (decide_local)
    bool &use_local = S.local_ok;          // turned on by decide_local, off by sort_flagged
    int *const rest = doubling ? &S.split_rest : (int *)nullptr;
    TiedList &L = B.L; const Workspace &w = B.w; const Tuning &tn = B.tn; const hipStream_t st = B.st;
    const int64_t m = L.m, n = B.n, tiles = ceil_div(m, RR_TILE);
    const int kb = K.kb, cap = tn.group_cap;          // cap: largest group ordered in LDS (C3: 1024 beats 512 by 1%)
    const unsigned gs_blocks = (unsigned)ceil_div(m, GS_TILE);
    uint32_t *const Valt = L.valt(w);
    uint8_t *const status = B.round_status_slab(K);        // != nullptr: the local pass writes status bytes there and no keys for the members it orders
    uint8_t *const flags = status ? status : (uint8_t *)L.Gn;      // where the local pass flags the members it leaves: the status bytes or L.Gn
    // groups of up to GB_CAP (8 192) members whose keys fit 32 bits: one workgroup each, in LDS (k_group_sort_big), on the list of
    // their first members that k_group_sort writes (L.Un is free until k_flag_gather); the rest goes through the global sort
    const bool big_local = !tn.no_big_group_sort && kb <= 32 && m > GS_CAP && !S.all_small;
    uint32_t *const bheads = big_local ? L.Un : (uint32_t *)nullptr, *const bcount = big_local ? w.total + RC_BIG_LISTED : (uint32_t *)nullptr;
    // the flagged members are sorted in the first `half` entries of L.rkB / Valt with the second half as the alternate
    // buffers: half is even (16-byte aligned 8-byte keys) and half + m_big never exceeds the n entries the slabs hold
    const size_t half = ((size_t)n / 2) & ~(size_t)1;
    Refined rf;
    int64_t m_flagged = -1, big_listed = -1;      // members the local pass left to the global sort (-1: no local pass ran), groups listed for k_group_sort_big (-1: not looked for)
    bool missed = false;                   // the deferred count was not zero, the global sort ran after all
    uint32_t words[ROUND_WORDS];           // the round's read-back: w.total and, where asked for, w.chg behind it
    uint32_t groups = 0;                   // groups of the list (count_groups)
    bool counted = false;                  // ... counted -- good until a local pass reuses w.tcnt / w.ft_cnt for its own compaction
    bool had_local_pass = false;           // launch_local_pass ran: the keys are in L.rkA already when the whole list goes through the global sort after all

    RefineRound(BuildCore &b, const KeyParams &pk, const KeySrc &k, RoundState &s, bool defer_ = false, bool doubling_ = false, bool retry_ = false)
        : B(b), Pk(pk), K(k), S(s), defer(defer_), doubling(doubling_), retry_local(retry_) { K.net_min = tn.network_min; }

    // sparse look-up: its own kernel, one suffix per thread (a chain of ~60 dependent loads each)
    int gather_sparse()
    {
        const int64_t gblocks = ceil_div(m, GK_THREADS);
        PROF(KC_GATHER, m, st, hipLaunchKernelGGL((k_gather_textkey<KS_SPARSE>), dim3((unsigned)(gblocks > 8192 ? 8192 : gblocks)), dim3(GK_THREADS), 0, st,
                                                  (const uint32_t *)L.V, L.G, B.dT, Pk, m, n, K, L.rkA));
        return SA_AMD_OK;
    }
    template <int M, bool STATUS, bool REFILL>
    int group_sort(uint8_t *fl, uint32_t *heads, uint32_t *count)
    {
        PROF(KC_LOCAL, m, st, hipLaunchKernelGGL((k_group_sort<M, STATUS, REFILL>), dim3(gs_blocks), dim3(GS_THREADS), 0, st, (const uint32_t *)L.V, L.G, L.U, B.dT, Pk, m, n, K,
                                                 L.rkA, L.V, fl, cap, heads, count));
        return SA_AMD_OK;
    }

    // how many groups has the list?  -> groups (w.total[RC_GROUPS]; w.ft_cnt: the exclusive group-start counts per tile)
    int count_groups()
    {
        PROF(KC_RR_COUNT, m, st, hipLaunchKernelGGL((k_flag_count<false>), dim3(rr_count_grid<false>(m)), dim3(RR_THREADS), 0, st,
                                                    (const uint8_t *)nullptr, L.U, L.G, m, w.tcnt, w.ft_cnt));
        PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan), dim3(1), dim3(SPINE_THREADS), 0, st, w.ft_cnt, w.thead, tiles, w.total + RC_GROUPS));
        counted = true;
        return read_words(&groups, w.total + RC_GROUPS, 4, st);
    }

    // The retry rule (doubling_rounds says when it is asked): the local pass is on again, in this round, when the average group fits a tile
    int decide_local()
    {
        if (use_local || !retry_local || tn.no_local_sort) return SA_AMD_OK;
        if (m < tn.dense_rekey_min) { use_local = true; return SA_AMD_OK; }      // (small lists do not count their groups)
        const int rc = count_groups();
        if (!rc && (int64_t)groups * 2 * tn.group_cap >= m) use_local = true;
        return rc;
    }

    // The local pass and, on the device, the counts of what it left: w.total[RC_FLAGGED] members, [RC_GROUPS] their groups, [RC_BIG_ORDERED]
    int launch_local_pass()
    {
        int rc;
        had_local_pass = true;
        if (!S.counters_clear) {
            HIP_TRY(hipMemsetAsync(w.total + RC_BIG_LISTED, 0, 8, st));           // [12] listed first members, [13] members ordered by k_group_sort_big
            HIP_TRY(hipMemsetAsync(w.total + RC_BIG_CLASS, 0, 8, st));            // [17], [18] listed groups of either k_group_sort_big instance
        }
        if (K.mode == KS_SPARSE && (rc = gather_sparse())) return rc;      // (then the sort on those keys: KS_PRE)
        if (status && tn.round_flags == 2) {
            // (diag library: what the round does not write must not be read -- a poisoned entry that is read changes the result)
            HIP_TRY(hipMemsetAsync(L.rkA, 0xEE, (size_t)m * 8, st));
            HIP_TRY(hipMemsetAsync(status, 0xFF, (((size_t)m + 7) & ~(size_t)7) + 8, st));
        }
        if (status) rc = by_mode<KS_RANK, KS_CHASE>(K.mode, [&](auto M) -> int { return group_sort<decltype(M)::value, true, false>(flags, bheads, bcount); });
        else        // (KS_SPARSE: the keys have just been gathered, KS_PRE)
            rc = by_mode<KS_PRE, KS_TEXT, KS_LOWKEY, KS_RANK, KS_CHASE>(K.mode, [&](auto M) -> int { return group_sort<decltype(M)::value, false, false>(flags, bheads, bcount); });
        if (rc) return rc;
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
        PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan_pair), dim3(2), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, w.total + RC_FLAGGED,
                                                       w.ft_cnt, (uint32_t *)nullptr, w.total + RC_GROUPS, tiles));
        return SA_AMD_OK;
    }

    // What the local pass left, by its counts (RC_WORDS words of w.total, read back by the caller): few flagged members go
    // through a global sort of their own and back to their places; too many send the whole list through it (sort_whole_list).
    int sort_flagged(const uint32_t *counts)
    {
        const int64_t m_big = counts[RC_FLAGGED], m_big_local = counts[RC_BIG_ORDERED];
        const uint32_t flagged_groups = counts[RC_GROUPS];
        m_flagged = m_big;
        big_listed = big_local ? (int64_t)counts[RC_BIG_LISTED] : -1;
        if ((size_t)m_big <= half && half + (size_t)m_big <= (size_t)n) {
            if (m_big > 0) {
                // groups no tile owns: global sort of (index of the group among them, key2), then back to their list positions
                // (a text that is one long run has ONE such group: no index bits at all, four passes instead of eight)
                const int idx_bits = bit_length((uint64_t)(flagged_groups > 0 ? flagged_groups - 1 : 0));
                PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((status ? k_flag_gather<true> : k_flag_gather<false>), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st,
                                                            (const uint8_t *)flags, (const uint64_t *)L.rkA, (const uint32_t *)L.V, L.U, L.G, m,
                                                            (const uint32_t *)w.tcnt, (const uint32_t *)w.ft_cnt, kb, L.rkB, Valt, L.Un));
                SortJob<uint64_t> big{ L.rkB, Valt, L.rkB + half, Valt + half, m_big, 0, kb + idx_bits };
                big.may_skip = true;
                SortResult<uint64_t> sr;
                const int rc = sort_pairs(big, w.ss, st, tn, &sr, &B.local);
                if (rc) return rc;
                PROF(KC_SCATTER, m_big, st, hipLaunchKernelGGL((k_scatter_back), dim3((unsigned)ceil_div(m_big, 256)), dim3(256), 0, st,
                                                               (const uint64_t *)sr.keys, (const uint32_t *)sr.vals,
                                                               (const uint32_t *)L.Un, L.G, kb, m_big, L.rkA, L.V));
            }
            rf.keys = L.rkA; rf.vals = L.V; rf.vnext = Valt; rf.m_global = m_big + m_big_local;      // (neither kind has been chased)
            rf.status = status;
            B.local.locally_sorted += m - m_big;
            if (m_big * 2 > m) use_local = false;           // mostly large groups: not worth another local pass
            return SA_AMD_OK;
        }
        if (m_big * 10 >= m * 9) use_local = false;     // (nearly) the whole list sits in groups no tile can own (runs, periodic texts): the next rounds skip the local pass
        if (status) {
            // The global sort below wants a key for EVERY member and the places the local pass owned have none: the pass runs again
            // in its key form for those places alone (k_group_sort REFILL, kernels/refine.hpp; DESIGN.md section 2, Status bytes), on
            // the order it left, which it does not change.  Every other place has the key the first launches left there.
            const int rc = by_mode<KS_RANK, KS_CHASE>(K.mode, [&](auto M) -> int { return group_sort<decltype(M)::value, false, true>(status, nullptr, nullptr); });
            if (rc) return rc;
        }
        return sort_whole_list();
    }

    // The whole list through the global sort.  Large lists are keyed by (index of the group in the list, key2) instead of (28-bit slot
    // of the group head, key2) when that saves radix passes: count the group heads first, then gather the keys in that form (k_gather_keyed)
    // or re-key the ones the local pass left (k_rekey_dense).  The head slots are not put back: the re-rank only compares neighbouring keys.
    int sort_whole_list()
    {
        int rc;
        int sort_bits = kb + B.g_bits;
        bool rekeyed = false;
        rf.status = nullptr;
        if (m >= tn.dense_rekey_min) {
            if ((!counted || had_local_pass) && (rc = count_groups())) return rc;
            const int idx_bits = bit_length((uint64_t)(groups > 0 ? groups - 1 : 0));
            if (ceil_div(kb + idx_bits, RADIX_BITS) < ceil_div(kb + B.g_bits, RADIX_BITS)) {
                sort_bits = kb + idx_bits;
                rekeyed = true;
            }
        }
        const bool split_wanted = rekeyed && !tn.no_split && m >= tn.split_min && groups > 0 && (int64_t)groups * tn.split_group_min <= m &&
                                  !(rest && *rest > 0);
        bool starts_ready = false;
        if (had_local_pass || K.mode == KS_SPARSE) {
            if (!had_local_pass && (rc = gather_sparse())) return rc;
            if (rekeyed)
                PROF(KC_RR_APPLY, m, st, hipLaunchKernelGGL((k_rekey_dense), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, L.rkA, L.U, L.G, m, (const uint32_t *)w.ft_cnt, kb));
        } else {
            const uint32_t *th = rekeyed ? (const uint32_t *)w.ft_cnt : (const uint32_t *)nullptr;
            // (when the three-way split may follow, the gather also writes its table of group starts: the first array in L.Gn)
            uint32_t *gs = split_wanted ? L.Gn : (uint32_t *)nullptr;
            starts_ready = gs != nullptr;
            rc = by_mode<KS_RANK, KS_TEXT, KS_LOWKEY>(K.mode, [&](auto M) -> int {
                PROF(KC_GATHER, m, st, hipLaunchKernelGGL((k_gather_keyed<decltype(M)::value>), dim3((unsigned)tiles), dim3(RR_THREADS), 0, st, (const uint32_t *)L.V, L.U, L.G, B.dT, Pk, m, n, K,
                                                          th, L.rkA, gs, groups));
                return SA_AMD_OK;
            });
            if (rc) return rc;
        }
        // Giant groups (runs, periodic texts, long repeats): all but a few members of a group carry the same key, so the few are pulled
        // out and sorted on their own and the rest only shifts (split_giant_groups) -- if its count pass finds them few; else the sort below
        if (rest && *rest > 0) --*rest;
        else if (split_wanted) {
            bool taken = false;
            rc = B.split_giant_groups(groups, kb, sort_bits, &rf, &taken, starts_ready);
            if (rc || taken) return rc;
            if (rest) *rest = 3;              // (a Fibonacci word's groups fall into parts of similar size round after round)
        }
        SortJob<uint64_t> whole{ L.rkA, L.V, L.rkB, Valt, m, 0, sort_bits };
        whole.may_skip = true;
        SortResult<uint64_t> sr;
        rc = sort_pairs(whole, w.ss, st, tn, &sr, &B.local);
        if (rc) return rc;
        rf.keys = sr.keys; rf.vals = sr.vals; rf.m_global = m;
        rf.vnext = (sr.vals == L.V) ? Valt : L.V;
        return SA_AMD_OK;
    }

    // Re-rank the order in rf -- gated while the round's mid-round count is deferred -- and read the round's words back, its one
    // read-back (words[RC_TIED]: members still tied).  ISA_MODE / PARENTS: the k_rr_apply / k_rr_count instantiation (3: text-keyed,
    // 1: sparse, 0: dense, 2: dense with binned ISA stores -- never deferred, its pairs are scattered behind the read-back).
    template <int ISA_MODE, bool PARENTS>
    int rerank(const uint32_t *gate)
    {
        int rc;
        RrApply a = B.round_args(rf);
        a.gate = gate; a.status = rf.status;
        if constexpr (ISA_MODE != 3) a.g_shift = B.key2_bits;
        if constexpr (ISA_MODE == 1) a.has_isa = w.has_isa;
        // dense rounds write a slot of SA once, in the round its suffix leaves the tied list (sa_final): the rounds go on until the list
        // is empty.  Sparse rounds look suffixes up in SA (sparse_key2): every round
        if constexpr (PARENTS) { a.tile_next = w.tnext; a.parent_tail = S.parent_tail ? 1 : 0; a.changed_cnt = w.chg; a.sa_final = tn.sa_every_round ? 0 : 1; }
        // a binned round: L.G has been consumed by the gather, the other key buffer by nothing -- they take the (suffix, rank) pairs
        if constexpr (ISA_MODE == 2) { a.pair_k = (rf.keys == L.rkA) ? L.rkB : L.rkA; a.pair_v = L.G; }
        // dense rounds: a group's rank is its last slot + 1 and a parent's last subgroup keeps it (k_rr_apply, TAIL); the tiles then also need the
        // first group start BEHIND them (second block of k_rr_scan_round).  rf.status: the group starts are read from the local pass's status bytes
        if constexpr (PARENTS)
            rc = rf.status ? B.rr_count<false, uint64_t, true, true>(rf.keys, L.U, m, w.tnext, B.key2_bits, gate, nullptr, nullptr, rf.status)
                           : B.rr_count<false, uint64_t, true>(rf.keys, L.U, m, w.tnext, B.key2_bits, gate);
        else rc = B.rr_count<false>(rf.keys, L.U, m, nullptr, 0, gate);
        if (rc) return rc;
        // (second block: the tiles' next group starts and the changed-rank counters of a dense round, the big-group counters saved and zeroed)
        PROF(KC_RR_SCAN, tiles, st, hipLaunchKernelGGL((k_rr_scan_round), dim3(2), dim3(SPINE_THREADS), 0, st, w.tcnt, w.thead, tiles, w.total,
                                                       PARENTS ? w.tnext : (uint32_t *)nullptr, PARENTS ? w.chg : (uint32_t *)nullptr, w.total + RC_BIG_LISTED, gate));
        if constexpr (PARENTS)
            rc = rf.status ? B.rr_apply<false, true, ISA_MODE, uint64_t, false, true>(rf.keys, a) : B.rr_apply<false, true, ISA_MODE>(rf.keys, a);
        else rc = B.rr_apply<false, true, ISA_MODE>(rf.keys, a);
        if (rc) return rc;
        if ((rc = read_words(words, w.total, PARENTS ? sizeof(words) : (size_t)RC_WORDS * 4, st))) return rc;      // (dense rounds: with w.chg)
        if constexpr (ISA_MODE == 2) {
            // (only the ranks that change became pairs; their number is in the counters)
            const int64_t pairs = chg_sum(words);
            if (pairs > 0 && (rc = scatter_binned(w.ss, w.isa, (uint32_t *)a.pair_k, a.pair_v, (uint32_t *)rf.keys, (uint32_t *)rf.vals, pairs, n, st, &B.local, tn))) return rc;
        }
        return SA_AMD_OK;
    }

    // The whole round, text-keyed or doubling; ISA_MODE == NO_RERANK: up to the re-rank, the counts read in the middle
    template <int ISA_MODE, bool PARENTS = false>
    int run()
    {
        int rc;
        if constexpr (ISA_MODE != NO_RERANK) {
            if (defer && use_local) {
                // deferred: the counts stay on the device, the re-rank kernels are gated on w.total[RC_FLAGGED] and everything is read at once
                if ((rc = launch_local_pass())) return rc;
                rf.keys = L.rkA; rf.vals = L.V; rf.vnext = Valt; rf.m_global = 0; rf.status = status;
                if ((rc = rerank<ISA_MODE, PARENTS>(w.total + RC_FLAGGED))) return rc;
                if (words[RC_FLAGGED] != 0) {
                    // a miss: the gated kernels did nothing; the words just read are the local pass's counts
                    missed = true;
                    return (rc = sort_flagged(words)) ? rc : rerank<ISA_MODE, PARENTS>(nullptr);
                }
                // as expected: the local pass ordered everything (what k_group_sort_big ordered was not chased: one look-up)
                m_flagged = 0;
                big_listed = S.all_small ? -1 : (int64_t)words[RC_BIG_LISTED_SAVED];
                rf.m_global = words[RC_BIG_ORDERED_SAVED];
                B.local.locally_sorted += m;
                return SA_AMD_OK;
            }
        }
        if ((rc = decide_local())) return rc;
        if (!use_local) rc = sort_whole_list();
        else if (!(rc = launch_local_pass()) && !(rc = read_words(words, w.total, (size_t)RC_WORDS * 4, st))) rc = sort_flagged(words);
        if constexpr (ISA_MODE != NO_RERANK) return rc ? rc : rerank<ISA_MODE, PARENTS>(nullptr);
        return rc;
    }
};

}  // namespace sa
