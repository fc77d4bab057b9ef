// kernels/lcp.hpp -- LCP array from a device-resident text and its suffix array.
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// Permuted LCP (Kärkkäinen, Manzini & Puglisi, CPM 2009), made data-parallel:
//   Φ[SA[i]] = SA[i-1]                       k_lcp_phi (or the binned scatter of host/pipeline.hpp)
//   j is REDUCIBLE iff j > 0, Φ[j] ∉ {0, n} and T[j-1] == T[Φ[j]-1]: then PLCP[j] = PLCP[j-1] - 1.  Every other position's
//   value h is compared directly (k_lcp_irreducible up to a per-lane cap, k_lcp_long / k_lcp_settle beyond it), and
//   v[j] = j + h is written over Φ[j] (0 where reducible).  The irreducible values sum to at most 2 n log2 n.
//   PLCP[j] + j never decreases and is constant along runs of reducible positions: an inclusive max-scan of v gives
//   PLCP[j] = M[j] - j (k_lcp_scan_spine + k_lcp_scan).
//   LCP[i] = PLCP[SA[i]], LCP[0] = 0                                       k_lcp_gather
//
// Text loads round a misaligned T down (up to three bytes in front of it, inside the same allocation) and never read a
// byte at or past T + n: the aligned word that holds the end is read byte by byte.
#pragma once
#include "common.hpp"

namespace sa {

constexpr int LCP_THREADS = 256;
constexpr int LCP_ITEMS = 8;
constexpr int LCP_TILE = LCP_THREADS * LCP_ITEMS;       // positions per tile of the irreducible pass and of the scan
constexpr int LCP_PIECE = 16;                            // bytes one lane compares per unit of the long compare
constexpr int LCP_SPINE_THREADS = 1024;
constexpr uint32_t LCP_NONE = 0xffffffffu;
constexpr int LCP_CAP_DEFAULT = 64;                      // bytes a lane compares before the pair goes to the long list (sa_amd_lcp_set_compare_cap)
constexpr int LCP_CAP_MAX = 1 << 20;

// control words (uint64) behind the sort scratch's error words, read back together with them
constexpr int LCP_C_LONG = 0, LCP_C_IRRED = 1, LCP_C_BYTES = 2, LCP_C_NEXT = 3, LCP_C_WORDS = 4;

// the aligned word at address a of the text [T, T + n): whole when it ends inside the text, else byte by byte up to T + n
__device__ __forceinline__ uint32_t lcp_aligned_word(uintptr_t a, uintptr_t end)
{
    if (a + 4 <= end) return *(const uint32_t *)a;
    uint32_t w = 0;
    for (int k = 0; k < 4; ++k)
        if (a + k < end) w |= (uint32_t)(*(const uint8_t *)(a + k)) << (8 * k);
    return w;
}

// the text from position p on, four bytes per next() (little-endian; bytes at or past n read as 0), one aligned load per step
struct LcpStream {
    uintptr_t a, end;
    uint32_t sh, cur;
    __device__ __forceinline__ LcpStream(const uint8_t *T, int64_t n, int64_t p)
    {
        const uintptr_t x = (uintptr_t)(T + p);
        a = x & ~(uintptr_t)3;
        end = (uintptr_t)(T + n);
        sh = (uint32_t)(x & 3u) * 8u;
        cur = lcp_aligned_word(a, end);
    }
    __device__ __forceinline__ uint32_t next()
    {
        a += 4;
        const uint32_t nxt = lcp_aligned_word(a, end);
        const uint32_t w = sh ? (cur >> sh) | (nxt << (32u - sh)) : cur;
        cur = nxt;
        return w;
    }
};

// one workgroup atomic per counter: the block sum of a 64-bit value
__device__ __forceinline__ void lcp_block_add(unsigned long long v, unsigned long long *dst)
{
    __shared__ unsigned long long s_sum[LCP_THREADS / WAVE];
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    __syncthreads();
    if (lane_id() == 0) s_sum[wave_id()] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < LCP_THREADS / WAVE; ++w) t += s_sum[w];
        if (t) atomicAdd(dst, t);
    }
}

// appends `want` lanes' values to list (wave-aggregated: one atomic per wave); returns the lane's slot or -1
__device__ __forceinline__ int64_t lcp_wave_append(bool want, uint32_t *cnt)
{
    const uint64_t m = __ballot(want);
    if (!m) return -1;
    const int leader = __builtin_ctzll(m);
    uint32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(cnt, (uint32_t)__popcll(m));
    base = __shfl(base, leader, WAVE);
    if (!want) return -1;
    const uint64_t below = m & ((1ull << lane_id()) - 1ull);
    return (int64_t)base + __popcll(below);
}

// Φ with plain stores (below the binned threshold): Φ[SA[i]] = SA[i-1], i = 1 .. n (SA[0] = n: Φ[SA[1]] = n)
__global__ __launch_bounds__(256) void k_lcp_phi(const uint32_t *__restrict__ SA, int64_t n, uint32_t *__restrict__ phi)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; i <= n; i += stride) {
        const uint32_t s = SA[i];
        if ((int64_t)s < n) phi[s] = SA[i - 1];
    }
}

// One lane per position j of the tile (strided by the workgroup size): reducible -> v = 0; irreducible -> h compared up to
// `cap` bytes, v = j + h; not settled within the cap -> j goes to the long list (Φ[j] stays in place for k_lcp_long) and
// v[j] is written by k_lcp_settle.  tile_max[tile] = max v of the tile; counters: irreducible positions, bytes loaded.
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_irreducible(const uint8_t *__restrict__ T, int64_t n, uint32_t *__restrict__ phi,
                                                                  int64_t cap, uint32_t *__restrict__ long_list, uint32_t *__restrict__ long_res,
                                                                  uint32_t *__restrict__ tile_max, unsigned long long *__restrict__ ctl)
{
    const int64_t base = (int64_t)blockIdx.x * LCP_TILE;
    uint32_t mx = 0;
    unsigned long long irr = 0, bytes = 0;
    for (int k = 0; k < LCP_ITEMS; ++k) {
        const int64_t j = base + (int64_t)k * LCP_THREADS + threadIdx.x;
        bool to_long = false;
        if (j < n) {
            int64_t p = phi[j];
            if (p > n) p = n;                                     // (SA not a permutation: any in-range value keeps the loads in bounds)
            uint32_t v = 0;
            const bool red = j > 0 && p != 0 && p != n && T[j - 1] == T[p - 1];
            if (!red) {
                ++irr;
                int64_t h = 0;
                if (p != n) {
                    const int64_t lim = n - (j > p ? j : p);
                    const int64_t stop = lim < cap ? lim : cap;
                    bool miss = false;
                    if (stop > 0) {
                        LcpStream A(T, n, j), B(T, n, p);
                        while (h < stop) {
                            const uint32_t x = A.next() ^ B.next();
                            bytes += 8;
                            if (x) { h += __builtin_ctz(x) >> 3; miss = true; break; }
                            h += 4;
                        }
                    }
                    if (miss || h >= lim) h = h < lim ? h : lim;
                    else to_long = true;                          // equal over the cap, the suffixes go on
                }
                v = (uint32_t)(j + h);
            }
            if (!to_long) { phi[j] = v; mx = mx > v ? mx : v; }
        }
        const int64_t slot = lcp_wave_append(to_long, (uint32_t *)&ctl[LCP_C_LONG]);
        if (slot >= 0) { long_list[slot] = (uint32_t)j; long_res[slot] = LCP_NONE; }
    }
    __shared__ uint32_t s_max[LCP_THREADS / WAVE + 1];
    uint32_t all;
    (void)block_incl_max<LCP_THREADS>(mx, s_max, &all);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = all;
    lcp_block_add(irr, &ctl[LCP_C_IRRED]);
    lcp_block_add(bytes, &ctl[LCP_C_BYTES]);
}

// One window [lo, lo + win) of every pair of the long list: units of LCP_PIECE bytes, consecutive lanes on consecutive pieces
// of one pair (a wave reads 1 KiB of each suffix); the first mismatch of a pair goes to res[k] by atomicMin.
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_long(const uint8_t *__restrict__ T, int64_t n, const uint32_t *__restrict__ phi,
                                                           const uint32_t *__restrict__ list, int64_t cnt, int64_t lo, int64_t win,
                                                           uint32_t *__restrict__ res, unsigned long long *__restrict__ ctl)
{
    const int64_t pieces = (win + LCP_PIECE - 1) / LCP_PIECE;
    const int64_t units = cnt * pieces;
    const int64_t stride = (int64_t)gridDim.x * LCP_THREADS;
    unsigned long long bytes = 0;
    for (int64_t u = (int64_t)blockIdx.x * LCP_THREADS + threadIdx.x; u < units; u += stride) {
        const int64_t k = u / pieces, q = u - k * pieces;
        const int64_t j = list[k];
        int64_t p = phi[j];
        if (p > n) p = n;
        const int64_t lim = n - (j > p ? j : p);
        const int64_t e = lo + win < lim ? lo + win : lim;
        const int64_t o = lo + q * LCP_PIECE;
        if (o >= e) continue;
        const int64_t len = e - o < LCP_PIECE ? e - o : LCP_PIECE;
        LcpStream A(T, n, j + o), B(T, n, p + o);
        for (int64_t d = 0; d < len; d += 4) {
            const uint32_t x = A.next() ^ B.next();
            bytes += 8;
            if (x) {
                const int64_t at = d + (__builtin_ctz(x) >> 3);
                if (at < len) atomicMin(&res[k], (uint32_t)(o + at));
                break;
            }
        }
    }
    lcp_block_add(bytes, &ctl[LCP_C_BYTES]);
}

// After a window: a pair with a mismatch, or whose shorter suffix ended inside the window, is settled (v[j] = j + h, the tile's
// maximum raised); the others go to the next list.
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_settle(int64_t n, uint32_t *__restrict__ phi, const uint32_t *__restrict__ list,
                                                             const uint32_t *__restrict__ res, int64_t cnt, int64_t end,
                                                             uint32_t *__restrict__ next_list, uint32_t *__restrict__ next_res,
                                                             uint32_t *__restrict__ tile_max, unsigned long long *__restrict__ ctl)
{
    const int64_t stride = (int64_t)gridDim.x * LCP_THREADS;
    const int64_t top = (cnt + stride - 1) / stride * stride;            // (whole waves in every iteration: the append is a wave op)
    for (int64_t k = (int64_t)blockIdx.x * LCP_THREADS + threadIdx.x; k < top; k += stride) {
        bool keep = false;
        int64_t j = 0;
        if (k < cnt) {
            j = list[k];
            int64_t p = phi[j];
            if (p > n) p = n;
            const int64_t lim = n - (j > p ? j : p);
            const uint32_t r = res[k];
            int64_t h = -1;
            if (r != LCP_NONE) h = r;
            else if (end >= lim) h = lim;
            else keep = true;
            if (h >= 0) {
                const uint32_t v = (uint32_t)(j + h);
                phi[j] = v;
                atomicMax(&tile_max[j / LCP_TILE], v);
            }
        }
        const int64_t slot = lcp_wave_append(keep, (uint32_t *)&ctl[LCP_C_NEXT]);
        if (slot >= 0) { next_list[slot] = (uint32_t)j; next_res[slot] = LCP_NONE; }
    }
}

// one workgroup: tile_max -> exclusive running maximum in place (the carry each tile of k_lcp_scan starts from)
__global__ __launch_bounds__(LCP_SPINE_THREADS) void k_lcp_scan_spine(uint32_t *__restrict__ tile_max, int64_t tiles)
{
    __shared__ uint32_t lds[LCP_SPINE_THREADS / WAVE + 1];
    __shared__ uint32_t s_inc[LCP_SPINE_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (tiles + LCP_SPINE_THREADS - 1) / LCP_SPINE_THREADS;
    int64_t b = (int64_t)t * per, e = b + per;
    if (b > tiles) b = tiles;
    if (e > tiles) e = tiles;
    uint32_t mx = 0;
    for (int64_t i = b; i < e; ++i) mx = max(mx, tile_max[i]);
    uint32_t all;
    s_inc[t] = block_incl_max<LCP_SPINE_THREADS>(mx, lds, &all);
    __syncthreads();
    uint32_t run = t ? s_inc[t - 1] : 0u;
    for (int64_t i = b; i < e; ++i) { const uint32_t m = tile_max[i]; tile_max[i] = run; run = max(run, m); }
}

// v -> PLCP in place: PLCP[j] = max(v[0..j]) - j.  A tile of LCP_TILE entries, LCP_ITEMS consecutive ones per thread
// (two 16-byte vectors), the carry of the tiles in front from k_lcp_scan_spine.  v must be 16-byte aligned.
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_scan(uint32_t *__restrict__ v, int64_t n, const uint32_t *__restrict__ carry)
{
    static_assert(LCP_ITEMS == 8, "two uint4 per thread");
    __shared__ uint32_t lds[LCP_THREADS / WAVE + 1];
    __shared__ uint32_t s_inc[LCP_THREADS];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * LCP_TILE + (int64_t)t * LCP_ITEMS;
    uint32_t x[LCP_ITEMS];
    if (j0 + LCP_ITEMS <= n) {
        const uint4 a = *(const uint4 *)(v + j0), b = *(const uint4 *)(v + j0 + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < LCP_ITEMS; ++k) x[k] = j0 + k < n ? v[j0 + k] : 0u;
    }
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < LCP_ITEMS; ++k) mx = max(mx, x[k]);
    uint32_t all;
    s_inc[t] = block_incl_max<LCP_THREADS>(mx, lds, &all);
    __syncthreads();
    uint32_t run = max(carry[blockIdx.x], t ? s_inc[t - 1] : 0u);
#pragma unroll
    for (int k = 0; k < LCP_ITEMS; ++k) { run = max(run, x[k]); x[k] = run - (uint32_t)(j0 + k); }
    if (j0 + LCP_ITEMS <= n) {
        *(uint4 *)(v + j0) = make_uint4(x[0], x[1], x[2], x[3]);
        *(uint4 *)(v + j0 + 4) = make_uint4(x[4], x[5], x[6], x[7]);
    } else {
#pragma unroll
        for (int k = 0; k < LCP_ITEMS; ++k) if (j0 + k < n) v[j0 + k] = x[k];
    }
}

// LCP[i] = PLCP[SA[i]], LCP[0] = 0 (an entry n outside slot 0 reads as 0: the range pass has already refused that array)
__global__ __launch_bounds__(256) void k_lcp_gather(const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ plcp,
                                                     uint32_t *__restrict__ LCP)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += stride) {
        const uint32_t s = i ? SA[i] : (uint32_t)n;
        LCP[i] = (int64_t)s < n ? plcp[s] : 0u;
    }
}

}  // namespace sa
