// kernels/doc_substrings.hpp -- document frequency of the repeated substrings: how many documents of the index's collection
// every suffix-tree node occurs in.  Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// Slots, LCP and nodes are those of kernels/substrings.hpp; prev is the collection's per-slot word of kernels/docs.hpp:
// prev[i] = previous slot of the same document + 1, 0 where there is none, 0xffffffff for slot 0.
//   A PAIR is (p, i) with p = prev[i] - 1 < i: two neighbouring occurrences of one document.  A node [lo, hi) holds
//   count - df pairs: every slot of it but the first of each document has its p inside.  The pair lies in exactly the nodes
//   that hold both slots, the ancestors-or-self of their lowest common node w, and depth(w) = min LCP(p, i].  Let m be ANY slot
//   of (p, i] where LCP has that minimum: m lies strictly inside w's interval, lo < m < hi, and so strictly inside every
//   ancestor's, but strictly inside no other node's -- everything strictly inside a deeper node is >= its depth > depth(w).
//   With G[m] = the pairs that chose m and E = the exclusive running sum of G (n + 2 entries):
//       df(node) = count - (E[hi] - E[lo + 1]).
//   Whichever argmin a lane takes, the sums are the same: no tie rule, and the integer atomics make G deterministic.
//
//   lz_rmq_query   argmin over [l, r] through the fan-out-32 minima that stage 1 of kernels/lz.hpp left (LzLevels).  The open
//                  range [a, b) of nodes climbs: at every level the nodes left of the first block edge (a .. a | 31, when a is
//                  not on an edge) and right of the last one (b & ~31 .. b - 1) are read, at most 31 a side; then a and b move
//                  to their parents.  When a and b - 1 share a block, its a .. b - 1 are read (at most 32) and the climb ends:
//                  at level K, the top, at the latest, where all nodes are one block.  The best node then descends to level 0,
//                  a block of 32 children a level, the last child taken unread.  A climb that ends at level j has loaded at
//                  most 62 j + 32 words and descends at most j levels: AT MOST 93 K + 32 WORDS A QUERY (404 at K = 4, 590 at
//                  K = 6, n < 2^31), whatever the array holds; every index is bounded by the levels' sizes, not by values.
//   k_dsub_pairs   one lane per slot: the pair, its argmin, G[m] += 1.  Pairs with a shallow lowest common node all hit one
//                  word of G, so equal targets inside a wave are combined first (a ballot loop: one atomic per distinct target).
//   k_dsub_scan    G -> E in place: tile sums, k_rep_sum_spine, the tiles again.
// The node pass and the gather with df are k_sub_nodes<WRITE, true> and k_sub_gather<true> of kernels/substrings.hpp.
#pragma once
#include "substrings.hpp"

namespace sa {

// control words (uint64) at byte 64 of the LCP control slab -- the LCP build's own words, dead once its front end is done
constexpr int DSUB_C_PAIRS = 2, DSUB_C_FAR = 3, DSUB_C_STEPS = 4, DSUB_C_RMAX = 5, DSUB_C_WORDS = 6;
static_assert(DSUB_C_DFSUM == 0 && DSUB_C_MAXDF == 1, "the node pass counts into the first two");

// A slot of [l, r] where A has its minimum over [l, r]; 0 <= l <= r < n.  lv: the minima of A[0 .. n).  steps: words loaded.
__device__ __forceinline__ int64_t lz_rmq_query(const uint32_t *__restrict__ A, int64_t n, const LzLevels &lv, int64_t l, int64_t r, uint32_t &steps)
{
    constexpr int64_t MASK = LZ_FAN - 1;
    int level = 0, blevel = 0;
    int64_t a = l, b = r + 1, bnode = l;
    uint32_t best = LZ_NONE;
    for (;;) {
        const uint32_t *w = level ? lv.base + lv.off[level] : A;
        if ((a >> LZ_FAN_LOG) == ((b - 1) >> LZ_FAN_LOG)) {
            for (int64_t j = a; j < b; ++j) { ++steps; const uint32_t v = w[j]; if (v < best) { best = v; bnode = j; blevel = level; } }
            break;
        }
        if (a & MASK) {
            const int64_t e = a | MASK;                       // (a's block lies in front of b - 1's: all of it exists)
            for (int64_t j = a; j <= e; ++j) { ++steps; const uint32_t v = w[j]; if (v < best) { best = v; bnode = j; blevel = level; } }
            a = e + 1;
        }
        if (b & MASK) {
            const int64_t s = b & ~MASK;
            for (int64_t j = s; j < b; ++j) { ++steps; const uint32_t v = w[j]; if (v < best) { best = v; bnode = j; blevel = level; } }
            b = s;
        }
        a >>= LZ_FAN_LOG;
        b >>= LZ_FAN_LOG;
        ++level;
        if (a >= b || level > lv.top) break;                  // nothing between the two fronts (the second: cannot be, the top is one block)
    }
    while (blevel > 0) {                                      // the first child of `bnode` that has its minimum
        --blevel;
        const uint32_t *w = blevel ? lv.base + lv.off[blevel] : A;
        const int64_t cnt = blevel ? lv.cnt[blevel] : n;
        const int64_t first = bnode << LZ_FAN_LOG;
        int64_t last = first + LZ_FAN - 1;
        if (last >= cnt) last = cnt - 1;
        int64_t c = first;
        for (; c < last; ++c) { ++steps; if (w[c] <= best) break; }
        bnode = c;                                            // (the last candidate is taken unread: it is the one)
    }
    return bnode;
}

// One lane per slot i of 1 .. n (N1 = n + 1): p = prev[i] - 1, checked p < i <= n before anything is read through it; m = an
// argmin of LCP over (p, i]; G[m] += 1.  COMBINE: lanes of a wave with the same m send one atomic.  Pairs, the pairs not inside
// one block of 32, the words loaded and the most one query loaded go to ctl (DSUB_C_*).  The workgroups walk over the slots
// (the trip count is the same for every lane of a wave: the ballots see whole waves) and count in registers, so the counters
// cost four atomics a workgroup and one a wave however long the text is -- one a wave and launch-sized workgroup, all on one
// cache line, took longer than the queries themselves.
template <bool COMBINE>
__global__ __launch_bounds__(LZ_THREADS) void k_dsub_pairs(const uint32_t *__restrict__ LCP, int64_t N1, const uint32_t *__restrict__ prev, LzLevels lv,
                                                            uint32_t *__restrict__ G, unsigned long long *__restrict__ ctl)
{
    const int64_t stride = (int64_t)gridDim.x * LZ_THREADS;
    unsigned long long pairs = 0, far = 0, total = 0;
    uint32_t worst = 0;
    for (int64_t base = (int64_t)blockIdx.x * LZ_THREADS; base < N1; base += stride) {
        const int64_t i = base + threadIdx.x;
        bool has = false;
        int64_t m = 0;
        uint32_t steps = 0;
        if (i >= 1 && i < N1) {
            const uint32_t w = prev[i];
            if (w != 0u && w != 0xffffffffu && (int64_t)w - 1 < i) {
                const int64_t p = (int64_t)w - 1;
                has = true;
                far += ((p + 1) >> LZ_FAN_LOG) != (i >> LZ_FAN_LOG) ? 1u : 0u;
                m = lz_rmq_query(LCP, N1, lv, p + 1, i, steps);
            }
        }
        if (COMBINE) {
            bool open = has;
            for (;;) {
                const unsigned long long todo = __ballot(open);
                if (!todo) break;
                const int leader = __ffsll((long long)todo) - 1;
                const int64_t tm = (int64_t)shfl64((uint64_t)m, leader);
                const bool same = open && m == tm;
                const unsigned long long group = __ballot(same);
                if (lane_id() == leader) atomicAdd(&G[tm], (uint32_t)__popcll(group));
                if (same) open = false;
            }
        } else if (has) {
            atomicAdd(&G[m], 1u);
        }
        pairs += has ? 1u : 0u;
        total += steps;
        worst = worst > steps ? worst : steps;
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) { const uint32_t w2 = __shfl_xor(worst, o, WAVE); worst = worst > w2 ? worst : w2; }
    if (lane_id() == 0 && worst) atomicMax(&ctl[DSUB_C_RMAX], (unsigned long long)worst);
    lcp_block_add(pairs, &ctl[DSUB_C_PAIRS]);
    lcp_block_add(far, &ctl[DSUB_C_FAR]);
    lcp_block_add(total, &ctl[DSUB_C_STEPS]);
}

// PHASE 0: cnt[tile] = sum of the tile of G.  PHASE 1: cnt holds the sums in front of every tile (k_rep_sum_spine): G <- its
// exclusive running sum, in place.  A thread owns REP_ITEMS consecutive words.
template <int PHASE>
__global__ __launch_bounds__(REP_THREADS) void k_dsub_scan(uint32_t *__restrict__ G, int64_t len, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    const int64_t j0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)threadIdx.x * REP_ITEMS;
    uint32_t x[REP_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) { x[k] = j0 + k < len ? G[j0 + k] : 0u; s += x[k]; }
    uint32_t total;
    const uint32_t ex = block_excl_sum<REP_THREADS>(s, lds, &total);
    if (PHASE == 0) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    } else {
        uint32_t run = cnt[blockIdx.x] + ex;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            if (j0 + k < len) G[j0 + k] = run;
            run += x[k];
        }
    }
}

}  // namespace sa
