// kernels/common.hpp -- wave / block scans, LDS-only barrier, global->LDS DMA helper.
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64); see DESIGN.md section 3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace sa {

constexpr int WAVE = 64;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & (WAVE - 1)); }
__device__ __forceinline__ int wave_id() { return (int)(threadIdx.x >> 6); }

// ------------------------------------------------------------------------------------------
// wave / block scans (wave64 shuffles, one LDS word per wave for the cross-wave step)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v)
{
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        uint32_t t = __shfl_up(v, o, WAVE);
        if (l >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v)
{
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        uint32_t t = __shfl_up(v, o, WAVE);
        if (l >= o) v = v > t ? v : t;
    }
    return v;
}

// 64-bit value of lane `src` (two 32-bit shuffles; executed by every lane of the wave)
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, WAVE) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, WAVE);
}

// Group-start flags: one byte per position of the sorted initial order, written by the last pass of the 64-bit initial sort
// (k_onesweep<..., HEAD_FLAGS>, kernels/onesweep.hpp) and read by the first re-rank (rr_lane_bits_flags, kernels/rerank.hpp)
// in place of the sorted keys.  A group = a maximal run of equal keys.
constexpr uint8_t OS_HF_SAME = 0;   // position p continues the group of p - 1
constexpr uint8_t OS_HF_START = 1;  // p starts a group (always so at p = 0)
constexpr uint8_t OS_HF_SEAM = 2;   // p is the first element of a tile's digit run: the pass could not see p - 1, but it stored the true
                                    // keys of p and p - 1 in its key buffer -- p starts a group iff they differ

// Status byte of a member of the tied list in a dense doubling round: written by the round's local pass (k_group_sort with STATUS,
// kernels/refine.hpp) per list PLACE, read by the round's re-rank (rr_lane_bits_status, kernels/rerank.hpp) in place of the
// 8-byte keys.  A group starts at place i iff  PHEAD(i) || (KEYED(i) ? keys[i] != keys[i - 1] : HEAD(i)).  A KEYED place that is no
// parent head has a KEYED place of the same parent group before it (ownership is per parent group), so both keys are true keys;
// no other entry of the key buffer is read, and the owned places have none.
constexpr uint8_t RS_PENDING = 1;   // member of a group no tile owned that is not ordered yet (k_flag_count / k_flag_gather; cleared by the kernels that order it)
constexpr uint8_t RS_KEYED = 2;     // the place was not owned by a tile of k_group_sort: keys[i] is its true key
constexpr uint8_t RS_HEAD = 4;      // owned places only: a group starts here in this round's order
constexpr uint8_t RS_PHEAD = 8;     // first place of its parent group (every place, owned or not)

// Exclusive block sum over THREADS threads; *total receives the block sum. lds: THREADS/64 + 1 words.
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t v, uint32_t *lds, uint32_t *total)
{
    constexpr int NW = THREADS / WAVE;
    const int l = lane_id(), w = wave_id();
    uint32_t inc = wave_incl_sum(v);
    if (l == WAVE - 1) lds[w] = inc;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        uint32_t s = lds[i];
        if (i < w) woff += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

// LDS-only workgroup barrier: orders LDS traffic (lgkmcnt) but, unlike __syncthreads(), does not drain the
// vector-memory counter -- a prefetch (global -> LDS DMA) or stores in flight stay in flight across it.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// global -> LDS DMA, BYTES per lane (4 or 16); the LDS destination is wave-uniform base + lane * BYTES
template <int BYTES>
__device__ __forceinline__ void glds(const void *src, void *lds_dst)
{
#if defined(__HIP_DEVICE_COMPILE__)      // the builtin exists in the device pass only
    if (BYTES == 16) __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void *)lds_dst, 16, 0, 0);
    else __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void *)lds_dst, 4, 0, 0);
#endif
}

// block_excl_sum with LDS-only barriers (RAW = true) or plain ones
template <int THREADS, bool RAW>
__device__ __forceinline__ uint32_t block_excl_sum_b(uint32_t v, uint32_t *lds, uint32_t *total)
{
    if (!RAW) return block_excl_sum<THREADS>(v, lds, total);
    constexpr int NW = THREADS / WAVE;
    const int l = lane_id(), w = wave_id();
    uint32_t inc = wave_incl_sum(v);
    if (l == WAVE - 1) lds[w] = inc;
    lds_barrier();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        uint32_t s = lds[i];
        if (i < w) woff += s;
        tot += s;
    }
    lds_barrier();
    *total = tot;
    return woff + inc - v;
}

// Inclusive block max-scan over THREADS threads; *total receives the block max. lds: THREADS/64 words.
template <int THREADS>
__device__ __forceinline__ uint32_t block_incl_max(uint32_t v, uint32_t *lds, uint32_t *total)
{
    constexpr int NW = THREADS / WAVE;
    const int l = lane_id(), w = wave_id();
    uint32_t inc = wave_incl_max(v);
    if (l == WAVE - 1) lds[w] = inc;
    __syncthreads();
    uint32_t wmax = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        uint32_t s = lds[i];
        if (i < w) wmax = wmax > s ? wmax : s;
        tot = tot > s ? tot : s;
    }
    __syncthreads();
    *total = tot;
    return inc > wmax ? inc : wmax;
}

}  // namespace sa
