// kernels/lds_sort.hpp -- the in-LDS sorting steps that several kernels share, each written once.
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64); see DESIGN.md section 3.
// Everything here is a __device__ __forceinline__ template: a kernel keeps its name, arguments, launch geometry and LDS arrays
// and hands the arrays in.  Users:
//   wave_digit_rank                  k_onesweep (onesweep.hpp), k_bucket_sort (bucket_sort.hpp), k_group_sort_big (refine.hpp);
//                                    diagnostic library: k_ss_bucket_sort (sample_sort.hpp), k_radix_downsweep_wcl (radix_sort_diag.hpp)
//   place_put / place_get            the same five kernels
//   lds_count_pass / lds_stable_pass k_bucket_sort (16-bit keys in LDS), k_group_sort_big (32-bit keys)
//   lds_bitonic_sort                 k_group_sort (the whole tile), k_group_sort_straddle (128 .. 1024 members)
//   count_rank_lt_le / chase_steps   k_group_sort and k_group_sort_straddle, KS_CHASE
// Not here, on purpose: sort_tile of radix_sort_diag.hpp (32-bit counts, ablation switches), induce_proto.hpp, the small-text
// kernel's own network (sm_bitonic_steps: swizzled layout, several steps per barrier), and the two passes of k_ss_bucket_sort
// (256-way stable digits owned by threads, plain barriers: sharing them would take a switch in the code below).
#pragma once
#include "common.hpp"

namespace sa {

// ---- stable rank of a key among the lanes of its wave that carry the same digit ----
// One ballot per digit bit leaves the mask of the valid lanes whose digit equals mine; mbcnt counts those below me.  my_hist is
// the wave's own row of 16-bit digit counts in LDS (what the wave's earlier items put into each digit): the first lane of a
// digit adds the digit's lanes to it.  Returns prior + below: my place among the wave's elements of digit d so far.  The caller
// keeps the items apart with __builtin_amdgcn_sched_barrier(0) (interleaving them only adds SGPR pressure).
template <int BITS>
__device__ __forceinline__ uint32_t wave_digit_rank(uint32_t d, bool ok, uint16_t *my_hist)
{
    const uint64_t okm = __ballot(ok);
    uint32_t xlo = ~(uint32_t)okm, xhi = ~(uint32_t)(okm >> 32);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const uint32_t sel = (uint32_t)((int32_t)(d << (31 - b)) >> 31);      // 0 or ~0: my bit b
        const uint64_t bal = __ballot(sel != 0);
        xlo |= (uint32_t)bal ^ sel;
        xhi |= (uint32_t)(bal >> 32) ^ sel;
    }
    const uint32_t mlo = ~xlo, mhi = ~xhi;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
    const uint32_t prior = my_hist[d];
    if (ok && below == 0) my_hist[d] = (uint16_t)(prior + (uint32_t)(__popc(mlo) + __popc(mhi)));
    return prior + below;
}

// ---- places below 65 536, two to a register: item j in half j & 1 of pp[j / 2] ----
// j is a constant of an unrolled loop.  place_put writes the items in ascending order (the even one sets the register), and is
// called unconditionally with a scalar: conditional element stores make the compiler keep a register array as a vector.
template <int N>
__device__ __forceinline__ void place_put(uint32_t (&pp)[N], int j, uint32_t r)
{
    if ((j & 1) == 0) pp[j >> 1] = r; else pp[j >> 1] |= r << 16;
}
template <int N>
__device__ __forceinline__ uint32_t place_get(const uint32_t (&pp)[N], int j)
{
    return (pp[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// ---- the LSD sort of a wave-striped segment in LDS, in two kinds of pass ----
// The segment has `size` <= THREADS * ITEMS elements; element e is held by wave e / (64 J), item (e / 64) % J, lane e % 64 with
// J = ceil(size / THREADS) items in use and e0 = wave * J * 64 + lane (so a stable rank inside the wave is a prefix count over
// lanes and items).  key / val are the caller's register arrays; both passes leave the elements in lds_k / lds_v in the new
// order, and the caller reloads them (behind a barrier) before the next pass.
//
// First pass, on the digit key & amask (< NB_A): one LDS counter per digit hands out the places, an exclusive scan of the counters
// in place says where each digit's run starts.  Which of two elements with the same digit comes first is left to the order the
// atomics arrive in -- enough when elements that agree in ALL sorted bits need no order among themselves.
template <int THREADS, int ITEMS, int NB_A, typename LdsKey>
__device__ __forceinline__ void lds_count_pass(const uint32_t (&key)[ITEMS], const uint32_t (&val)[ITEMS], uint32_t (&pp)[ITEMS / 2],
                                               int J, int e0, int size, uint32_t amask,
                                               LdsKey *lds_k, uint32_t *lds_v, uint32_t *cnt_a, uint32_t *scan_lds)
{
    static_assert(NB_A % THREADS == 0 || THREADS % NB_A == 0, "the counters are scanned by the whole workgroup");
    const int tid = threadIdx.x;
    for (int i = tid; i < NB_A; i += THREADS) cnt_a[i] = 0;
    __syncthreads();                               // (also: the caller's loads have arrived)
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        uint32_t r = 0;
        if (j < J && (e0 + j * WAVE) < size) r = atomicAdd(&cnt_a[key[j] & amask], 1u);
        place_put(pp, j, r);
    }
    lds_barrier();
    {
        // exclusive sums over the NB_A counters, in place
        constexpr int BPT = NB_A >= THREADS ? NB_A / THREADS : 1;
        const bool scans = NB_A >= THREADS || tid < NB_A;
        uint32_t c[BPT], sum = 0;
#pragma unroll
        for (int i = 0; i < BPT; ++i) { c[i] = scans ? cnt_a[tid * BPT + i] : 0u; sum += c[i]; }
        uint32_t all;
        uint32_t run = block_excl_sum_b<THREADS, true>(sum, scan_lds, &all);
#pragma unroll
        for (int i = 0; i < BPT; ++i) { if (scans) cnt_a[tid * BPT + i] = run; run += c[i]; }
    }
    lds_barrier();
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        if (j < J && (e0 + j * WAVE) < size) {
            const uint32_t ps = place_get(pp, j) + cnt_a[key[j] & amask];
            lds_k[ps] = (LdsKey)key[j];
            lds_v[ps] = val[j];
        }
    }
}

// Stable pass, on the digit (key >> shift) & dmask of at most BBITS bits (2^BBITS = 64: lane d of wave 0 owns digit d): zero the
// per-wave digit counts, rank inside the wave (wave_digit_rank), wave 0 turns the counts into per-wave offsets and the digits'
// starts, every element goes to start of its digit + offset of its wave + rank.
template <int THREADS, int ITEMS, int BBITS, typename LdsKey>
__device__ __forceinline__ void lds_stable_pass(const uint32_t (&key)[ITEMS], const uint32_t (&val)[ITEMS], uint32_t (&pp)[ITEMS / 2],
                                                int J, int e0, int size, int shift, uint32_t dmask,
                                                LdsKey *lds_k, uint32_t *lds_v, uint16_t (*wave_hist)[1 << BBITS], uint32_t *digit_base)
{
    constexpr int NWAVES = THREADS / WAVE, NB_B = 1 << BBITS;
    static_assert(NB_B == WAVE, "lane d of wave 0 owns digit d");
    const int tid = threadIdx.x, l = lane_id(), w = wave_id();
    uint16_t *my_hist = wave_hist[w];
    for (int i = tid; i < NWAVES * NB_B / 2; i += THREADS) ((uint32_t *)&wave_hist[0][0])[i] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        uint32_t r = 0;
        if (j < J) {                               // (uniform)
            r = wave_digit_rank<BBITS>((key[j] >> shift) & dmask, (e0 + j * WAVE) < size, my_hist);
            __builtin_amdgcn_sched_barrier(0);
        }
        place_put(pp, j, r);
    }
    lds_barrier();
    // ---- wave 0, lane d: per-wave offsets of digit d, its start in the segment ----
    if (w == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int ww = 0; ww < NWAVES; ++ww) {
            const uint32_t cnt = wave_hist[ww][l];
            wave_hist[ww][l] = (uint16_t)tot;
            tot += cnt;
        }
        digit_base[l] = wave_incl_sum(tot) - tot;
    }
    lds_barrier();
    // ---- into LDS in the order of this digit (stable) ----
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        if (j < J && (e0 + j * WAVE) < size) {
            const uint32_t d = (key[j] >> shift) & dmask;
            const uint32_t ps = place_get(pp, j) + digit_base[d] + my_hist[d];
            lds_k[ps] = (LdsKey)key[j];
            lds_v[ps] = val[j];
        }
    }
}

// ---- bitonic network over P 8-byte composites in LDS, ascending; P a power of two, 128 <= P <= MAX_P; t = threadIdx.x < THREADS ----
// Exchange x of a step of distance j pairs lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)) with lo | j, and thread t takes the
// exchanges x = t + i * THREADS.  While j <= 64, lo and lo | j lie in the 128-element block x / 64 (lo / 128 = x / 64 once j
// divides 64).  THREADS is a multiple of 64, so the 64 lanes of a wave hold 64 CONSECUTIVE exchanges starting at a multiple of
// 64 in every round i: exactly one such block, and the same blocks in every step.  A run of steps of distance <= 64 therefore
// only reads what the wave itself wrote: it needs the wave's own LDS traffic to have landed (s_waitcnt), not a workgroup
// barrier -- 56 of the 66 steps at P = 2048.  A barrier stands wherever this step or the next has a distance above 64, and
// behind the last step.  This rests on the x = t + i * THREADS indexing: give a thread consecutive exchanges instead
// (x = t * n + i), or let a wave's lanes interleave with another wave's, and a wave's 64 exchanges spread over several blocks
// that other waves write in the same step -- the barrier-free steps then read stale elements.
// MAX_P (the array's size) bounds the rounds at compile time: they are unrolled, each guarded by x < P / 2.
template <int THREADS, int MAX_P>
__device__ __forceinline__ void lds_bitonic_sort(uint64_t *s_key, int P, int t)
{
    static_assert(THREADS % WAVE == 0, "a wave's exchanges of one round are 64 consecutive ones from a multiple of 64: one 128-element block");
    static_assert(WAVE == 64, "the barrier-free distance (64) is half the block that 64 exchanges cover");
    static_assert(MAX_P >= 2 * WAVE && (MAX_P & (MAX_P - 1)) == 0 && (MAX_P / 2) % THREADS == 0, "whole rounds of THREADS exchanges");
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < MAX_P / 2 / THREADS; ++i) {
                const int x = t + i * THREADS;
                if (x < P / 2) {
                    const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
                    const uint64_t a = s_key[lo], c = s_key[hi];
                    if ((a > c) == ((lo & k) == 0)) { s_key[lo] = c; s_key[hi] = a; }
                }
            }
            const int next_j = j > 1 ? (j >> 1) : k;                 // (the next step's distance; behind the last step: a barrier)
            if (j > WAVE || next_j > WAVE || (j == 1 && k == P)) __syncthreads();
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
}

// ---- the chase (KS_CHASE): composites (key << POS_BITS | place) in s_key ----
// Among s_key[a .. a + e): rank = composites below `mine` (the member's new place in the subgroup: composites are distinct),
// lt / le = members whose key is smaller than / at most `comp`, the key of `mine` (the extent of the member's new subgroup:
// first place a + lt, le - lt members).
template <int POS_BITS>
__device__ __forceinline__ void count_rank_lt_le(const uint64_t *s_key, int a, int e, uint64_t mine, uint64_t comp, int &rank, int &lt, int &le)
{
    rank = 0; lt = 0; le = 0;
    for (int i = a; i < a + e; ++i) {
        const uint64_t k = s_key[i];
        rank += k < mine ? 1 : 0;
        lt += (k >> POS_BITS) < comp ? 1 : 0;
        le += (k >> POS_BITS) <= comp ? 1 : 0;
    }
}

// Steps 2 .. iters of the chase.  Before: the `size` members sit at their places of the first step in val_cur, the subgroup of
// each (first place << 16 | members) in rng[0]; the caller has put a barrier behind those stores.  Every step touches only the
// members whose subgroup still has more than one member: they fetch the rank of the suffix it * h symbols further on, count
// inside their subgroup and move to their new place in val_nxt / the other row of rng; then the buffers change roles.  Ends
// early when nothing is tied.  Returns the row of rng that holds the result; the values are in val_cur when it is 0, else in
// val_nxt.  (size = THREADS * ITEMS as a constant folds the guards away.)
template <int THREADS, int ITEMS, int POS_BITS>
__device__ __forceinline__ int chase_steps(uint64_t *s_key, uint32_t *val_cur, uint32_t *val_nxt, uint32_t (*rng)[THREADS * ITEMS],
                                           int size, int t, int iters, int64_t h, const uint32_t *isa, int64_t n)
{
    static_assert(THREADS * ITEMS <= (1 << POS_BITS), "a place fits into POS_BITS bits");
    int cur = 0;
    for (int it = 2; it <= iters; ++it) {
        uint32_t rg[ITEMS], vq[ITEMS];
        uint64_t mine[ITEMS];
        bool any = false;
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int q = r * THREADS + t;
            rg[r] = q < size ? rng[cur][q] : 1u;
            vq[r] = q < size ? val_cur[q] : 0u;
            any |= (rg[r] & 0xffffu) > 1u;
        }
        if (!__syncthreads_or(any)) break;
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int q = r * THREADS + t;
            mine[r] = 0;
            if ((rg[r] & 0xffffu) > 1u) {
                const int64_t p = (int64_t)vq[r] + (int64_t)it * h;
                const uint64_t comp = p < n ? (uint64_t)n + (uint64_t)isa[p] : (uint64_t)(n - 1 - (int64_t)vq[r]);
                mine[r] = (comp << POS_BITS) | (uint64_t)q;
                s_key[q] = mine[r];
            }
        }
        __syncthreads();
        const int nxt = cur ^ 1;
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int q = r * THREADS + t;
            if (q >= size) continue;
            const int e = (int)(rg[r] & 0xffffu), a = (int)(rg[r] >> 16);
            if (e > 1) {
                int rank, lt, le;
                count_rank_lt_le<POS_BITS>(s_key, a, e, mine[r], mine[r] >> POS_BITS, rank, lt, le);
                val_nxt[a + rank] = vq[r];
                rng[nxt][a + rank] = ((uint32_t)(a + lt) << 16) | (uint32_t)(le - lt);
            } else {
                val_nxt[q] = vq[r];
                rng[nxt][q] = rg[r];
            }
        }
        __syncthreads();
        { uint32_t *tmp = val_cur; val_cur = val_nxt; val_nxt = tmp; }
        cur = nxt;
    }
    return cur;
}

}  // namespace sa
