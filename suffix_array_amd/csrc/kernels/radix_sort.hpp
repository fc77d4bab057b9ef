// kernels/radix_sort.hpp -- what the product launches of the LSD radix sort besides the single-pass tile scatter (kernels/onesweep.hpp):
// the digit geometry, digit extraction and the counting kernels (first pass of a sort whose producer did not count, the pass
// behind a skipped one).  The rest of the three-kernel pass of rounds 1-2 is in kernels/radix_sort_diag.hpp (diagnostic library).
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64); see DESIGN.md section 3.
#pragma once
#include "common.hpp"

namespace sa {

// stable LSD radix sort of (key, u32 value) pairs, 8-bit digits
constexpr int RADIX_BITS = 8;
constexpr int RADIX = 1 << RADIX_BITS;
constexpr int SORT_THREADS = 256;
constexpr int SORT_WAVES = SORT_THREADS / WAVE;

__device__ __forceinline__ uint32_t digit_of(uint64_t key, int shift, uint32_t dmask)
{
    return (uint32_t)(key >> shift) & dmask;
}
__device__ __forceinline__ uint32_t digit_of(uint32_t key, int shift, uint32_t dmask)
{
    return (key >> shift) & dmask;
}

__global__ __launch_bounds__(SORT_THREADS) void k_radix_upsweep(const uint64_t *__restrict__ keys,
                                                                 uint32_t *__restrict__ counts, int64_t n,
                                                                 int shift, uint32_t dmask,
                                                                 int64_t chunk_elems, int G, int split,
                                                                 int64_t sub_elems)
{
    __shared__ uint32_t h[SORT_WAVES][RADIX];
    for (int i = threadIdx.x; i < SORT_WAVES * RADIX; i += SORT_THREADS) (&h[0][0])[i] = 0;
    __syncthreads();
    uint32_t *mine = h[wave_id()];
    // `split` workgroups share one downsweep chunk (more waves in flight for the streaming read);
    // sub_elems is even, so every part starts 16-byte aligned
    const int g = (int)(blockIdx.x / split), part = (int)(blockIdx.x % split);
    const int64_t cbegin = (int64_t)g * chunk_elems;
    int64_t cend = cbegin + chunk_elems;
    if (cend > n) cend = n;
    int64_t begin = cbegin + (int64_t)part * sub_elems;
    int64_t end = begin + sub_elems;
    if (begin > cend) begin = cend;
    if (end > cend || part == split - 1) end = cend;
    // two keys (16 B) per lane per load, four loads in flight per lane; chunk_elems is a multiple of
    // the tile size so the pairs are 16-byte aligned
    const int64_t npair = (end - begin) / 2;
    const ulonglong2 *K2 = (const ulonglong2 *)(keys + begin);
    auto count2 = [&](const ulonglong2 &q) {
        const uint32_t d0 = digit_of((uint64_t)q.x, shift, dmask), d1 = digit_of((uint64_t)q.y, shift, dmask);
        // constant digits (all-equal high bits) would serialise the LDS atomic 64 ways
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0);
        const uint64_t act = __ballot(1);                          // evaluated by every active lane
        if (__all(d0 == f && d1 == f)) {
            // the lowest ACTIVE lane adds for the wave (lane 0 may have left the loop already)
            if (lane_id() == __ffsll((unsigned long long)act) - 1) atomicAdd(&mine[f], 2u * (uint32_t)__popcll(act));
        } else {
            atomicAdd(&mine[d0], 1u);
            atomicAdd(&mine[d1], 1u);
        }
    };
    int64_t i = threadIdx.x;
    for (; i + 3 * SORT_THREADS < npair; i += 4 * SORT_THREADS) {
        const ulonglong2 q0 = K2[i], q1 = K2[i + SORT_THREADS], q2 = K2[i + 2 * SORT_THREADS], q3 = K2[i + 3 * SORT_THREADS];
        count2(q0); count2(q1); count2(q2); count2(q3);
    }
    for (; i < npair; i += SORT_THREADS) count2(K2[i]);
    if (((end - begin) & 1) && threadIdx.x == 0) atomicAdd(&mine[digit_of(keys[end - 1], shift, dmask)], 1u);
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) s += h[w][threadIdx.x];
    if (split == 1) counts[(int64_t)threadIdx.x * G + g] = s;
    else if (s) atomicAdd(&counts[(int64_t)threadIdx.x * G + g], s);     // counts zeroed by the host
}

constexpr int SPINE_THREADS = 1024;       // one block scans a row of per-tile counts (kernels/rerank.hpp; the spine of radix_sort_diag.hpp)

// the same for 32-bit keys (two-stage initial sort: only the top 32 key bits are sorted), four keys per 16-byte load
__global__ __launch_bounds__(SORT_THREADS) void k_radix_upsweep32(const uint32_t *__restrict__ keys,
                                                                   uint32_t *__restrict__ counts, int64_t n,
                                                                   int shift, uint32_t dmask,
                                                                   int64_t chunk_elems, int G, int split,
                                                                   int64_t sub_elems)
{
    __shared__ uint32_t h[SORT_WAVES][RADIX];
    for (int i = threadIdx.x; i < SORT_WAVES * RADIX; i += SORT_THREADS) (&h[0][0])[i] = 0;
    __syncthreads();
    uint32_t *mine = h[wave_id()];
    const int g = (int)(blockIdx.x / split), part = (int)(blockIdx.x % split);
    const int64_t cbegin = (int64_t)g * chunk_elems;
    int64_t cend = cbegin + chunk_elems;
    if (cend > n) cend = n;
    int64_t begin = cbegin + (int64_t)part * sub_elems;      // sub_elems is a multiple of 4: 16-byte aligned parts
    int64_t end = begin + sub_elems;
    if (begin > cend) begin = cend;
    if (end > cend || part == split - 1) end = cend;
    const int64_t nquad = (end - begin) / 4;
    const uint4 *K4 = (const uint4 *)(keys + begin);
    auto count4 = [&](const uint4 &q) {
        const uint32_t d0 = digit_of((uint32_t)q.x, shift, dmask), d1 = digit_of((uint32_t)q.y, shift, dmask);
        const uint32_t d2 = digit_of((uint32_t)q.z, shift, dmask), d3 = digit_of((uint32_t)q.w, shift, dmask);
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0);
        const uint64_t act = __ballot(1);
        if (__all(d0 == f && d1 == f && d2 == f && d3 == f)) {
            if (lane_id() == __ffsll((unsigned long long)act) - 1) atomicAdd(&mine[f], 4u * (uint32_t)__popcll(act));
        } else {
            atomicAdd(&mine[d0], 1u); atomicAdd(&mine[d1], 1u); atomicAdd(&mine[d2], 1u); atomicAdd(&mine[d3], 1u);
        }
    };
    int64_t i = threadIdx.x;
    for (; i + 3 * SORT_THREADS < nquad; i += 4 * SORT_THREADS) {
        const uint4 q0 = K4[i], q1 = K4[i + SORT_THREADS], q2 = K4[i + 2 * SORT_THREADS], q3 = K4[i + 3 * SORT_THREADS];
        count4(q0); count4(q1); count4(q2); count4(q3);
    }
    for (; i < nquad; i += SORT_THREADS) count4(K4[i]);
    if (threadIdx.x == 0)
        for (int64_t t = begin + nquad * 4; t < end; ++t) atomicAdd(&mine[digit_of(keys[t], shift, dmask)], 1u);
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) s += h[w][threadIdx.x];
    if (split == 1) counts[(int64_t)threadIdx.x * G + g] = s;
    else if (s) atomicAdd(&counts[(int64_t)threadIdx.x * G + g], s);
}

#ifdef SA_AMD_DIAG
// diagnostic library only (phase stamps of k_radix_downsweep_wcl, k_onesweep and k_group_sort): cycles of wave 0 per phase, summed
// over tiles and workgroups
__device__ unsigned long long g_phase_cycles[16];
__device__ int g_gs_stamp_on;          // k_group_sort adds its per-phase cycles (wave 0) to g_phase_cycles[8..15]
__device__ int g_rr_stamp_on;          // k_rr_count adds its per-phase cycles (wave 0) to g_phase_cycles[0..7] (tools/rr_count_stamps.py)
#endif

}  // namespace sa
