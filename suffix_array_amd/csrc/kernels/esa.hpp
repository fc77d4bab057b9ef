// kernels/esa.hpp -- enhanced suffix array: the LCP table of a fixed search tree over the suffix array, and the batched search
// that uses it (Manber & Myers, SIAM J. Comput. 1993).  Part of the MI355X-native suffix-array engine
// (gfx950 / CDNA4, wave64).
//
// The tree is an ALIGNED bisection over the N = n + 1 slots, shifted by one: slot m is node x = m + 1, x = 0 is a virtual
// -inf suffix and x >= N + 1 are virtual +inf suffixes.  The search keeps an open interval (L, R), starts at (0, P) with P the
// smallest power of two >= N + 1 and probes x = (L + R) / 2, so every real node x has the fixed interval (x - h, x + h),
// h = lowbit(x), and with B[z] = LCP[z] (z < N), 0 (z >= N):
//   Llcp[x] = lcp(suf(x - h), suf(x)) = min B[x - h .. x - 1]        Rlcp[x] = lcp(suf(x), suf(x + h)) = min B[x .. x + h - 1]
// the two halves of the aligned block of 2h at x - h.  pair[x - 1] = Llcp | Rlcp << 32: one 8-byte load per step.
#pragma once
#include "common.hpp"
#include "extras.hpp"
#include "sym.hpp"

namespace sa {

constexpr int ESA_THREADS = 256;
constexpr int ESA_TILE_LOG = 12;
constexpr int ESA_TILE = 1 << ESA_TILE_LOG;         // entries per tile: levels 1..12 of the tree inside one tile (16 KiB of LDS)

// One pass of the table build.  src holds B (shift 0) or the tile minima of the previous pass (shift 12, 24): tile t of this
// pass covers src[t * 4096 .. t * 4096 + 4095] (entries at or past src_len read as 0) and owns every node whose aligned block
// lies inside it, i.e. tile-local y = h (2k + 1) with h <= 2048.  Node y of this pass is node x = (t * 4096 + y) << shift of the
// tree; its pair goes to pair[x - 1] when 1 <= x <= N.  The tile's minimum goes to tile_min[t] (nullptr: not needed).
__global__ __launch_bounds__(ESA_THREADS) void k_esa_tree(const uint32_t *__restrict__ src, int64_t src_len, int shift, int64_t N,
                                                          uint64_t *__restrict__ pair, uint32_t *__restrict__ tile_min)
{
    __shared__ uint32_t a[ESA_TILE];                // after level j: a[k 2^j] = min of the aligned block [k 2^j, (k + 1) 2^j)
    __shared__ uint64_t pr[ESA_TILE];               // the pair of tile-local node y (pr[0]: a node of a later pass)
    const int64_t base = (int64_t)blockIdx.x * ESA_TILE;
    for (int k = threadIdx.x; k < ESA_TILE; k += ESA_THREADS)
        a[k] = base + k < src_len ? src[base + k] : 0u;
    __syncthreads();
    for (int j = 1; j <= ESA_TILE_LOG; ++j) {
        const int h = 1 << (j - 1), nodes = ESA_TILE >> j;
        for (int k = threadIdx.x; k < nodes; k += ESA_THREADS) {
            const int y = h * (2 * k + 1);
            const uint32_t lo = a[y - h], hi = a[y];
            pr[y] = (uint64_t)lo | ((uint64_t)hi << 32);
            a[y - h] = lo < hi ? lo : hi;
        }
        __syncthreads();
    }
    for (int y = threadIdx.x; y < ESA_TILE; y += ESA_THREADS) {
        const int64_t x = (base + y) << shift;
        if (y > 0 && x <= N) pair[x - 1] = pr[y];
    }
    if (threadIdx.x == 0 && tile_min) tile_min[blockIdx.x] = a[0];
}

struct EsaState { uint64_t L; int64_t l, r; };       // the final left end and lcp(pat, suf(L)), lcp(pat, suf(R)) (R = L + 1)

// One Manber-Myers descent over the fixed tree, log_p steps.  UPPER = false: the lower bound of pat (a suffix equal to pat is
// not smaller); UPPER = true: the lower bound of pat followed by +inf (a suffix that starts with pat is smaller).  l and r stay
// exact, max(l, r) never decreases, and a step compares text only when the table leaves the order open.
template <bool UPPER>
__device__ __forceinline__ EsaState esa_descent(const uint8_t *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n,
                                                const uint64_t *__restrict__ pair, int log_p, const uint8_t *__restrict__ pat,
                                                int64_t plen, int64_t *bytes, int64_t *table_steps)
{
    const uint64_t N = (uint64_t)n + 1;
    uint64_t L = 0, R = 1ull << log_p;
    int64_t l = 0, r = 0;
    for (int s = 0; s < log_p; ++s) {
        const uint64_t x = (L + R) >> 1;
        bool right = false;
        int64_t c0 = -1;                                     // >= 0: compare from there
        if (x > N) { right = false; r = 0; ++*table_steps; }  // a virtual +inf suffix
        else {
            const uint64_t pq = pair[x - 1];
            if (l >= r) {
                const int64_t t = (int64_t)(uint32_t)pq;     // Llcp
                if (t > l) right = true;
                else if (t < l) { right = false; r = t; }
                else c0 = l;
            } else {
                const int64_t t = (int64_t)(uint32_t)(pq >> 32);   // Rlcp
                if (t > r) right = false;
                else if (t < r) { right = true; l = t; }
                else c0 = r;
            }
            if (c0 >= 0) {
                const SuffixCmp c = wave_compare_from(T, n, (int64_t)SA[x - 1], pat, plen, c0, bytes);
                right = c.ord < 0 || (UPPER && (int64_t)c.lcp == plen);
                if (right) l = c.lcp; else r = c.lcp;
            } else {
                ++*table_steps;
            }
        }
        if (right) L = x; else R = x;
    }
    EsaState st; st.L = L; st.l = l; st.r = r;
    return st;
}

// The batched search of k_search_batch (same outputs, bit for bit) over the pair table, one wave per pattern.  range_lo is the
// left end of descent 1, range_hi that of descent 2; search_lcp takes the branches of k_search_batch with descent 1's l and r
// standing in for the lcps of SA[i - 1] and SA[i].  stats (3 counters: compared bytes, steps, table steps) or nullptr.
__global__ __launch_bounds__(SEARCH_THREADS) void k_esa_search(
    const uint8_t *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint64_t *__restrict__ pair, int log_p,
    const uint8_t *__restrict__ pat_data, const int64_t *__restrict__ pat_off, int32_t count, uint8_t *__restrict__ contains,
    uint32_t *__restrict__ range_lo, uint32_t *__restrict__ range_hi, uint32_t *__restrict__ lcp_start, uint32_t *__restrict__ lcp_len,
    const uint32_t *__restrict__ bkt, unsigned long long *__restrict__ stats)
{
    const int q = (int)((blockIdx.x * (int64_t)SEARCH_THREADS + threadIdx.x) / WAVE);
    if (q >= count) return;                                   // whole waves leave together
    const uint8_t *pat = pat_data + pat_off[q];
    const int64_t plen = pat_off[q + 1] - pat_off[q];
    const int64_t len = n + 1;
    int64_t bytes = 0, table_steps = 0;
    const EsaState a = esa_descent<false>(T, SA, n, pair, log_p, pat, plen, &bytes, &table_steps);
    const EsaState b = esa_descent<true>(T, SA, n, pair, log_p, pat, plen, &bytes, &table_steps);
    const int64_t i = (int64_t)a.L, j = (int64_t)b.L;
    bool empty_bucket = false;                                // the reference's search_lcp with buckets (src/sa.rs:211-222)
    if (bkt && plen > 1) {
        const int idx = (int)pat[0] * 257 + (int)pat[1] + 2;
        empty_bucket = bkt[idx - 1] == bkt[idx];
    } else if (bkt && plen == 1) {
        empty_bucket = bkt[(int)pat[0] * 257] == bkt[(int)pat[0] * 257 + 257];
    }
    uint32_t ls = (uint32_t)n, ll = 0;
    if (empty_bucket) {
        const int64_t tlo = bkt[(int)pat[0] * 257], thi = bkt[(int)pat[0] * 257 + 257];
        if (thi > tlo) { ls = SA[tlo]; ll = 1; }
    } else if (i < len && a.r == plen && n - (int64_t)SA[i] == plen) {
        ls = SA[i]; ll = (uint32_t)plen;                      // Ok(i): start..s.len()
    } else if (i > 0 && i < len) {
        if (a.l > a.r) { ls = SA[i - 1]; ll = (uint32_t)a.l; } else { ls = SA[i]; ll = (uint32_t)a.r; }
    } else if (i == 0) { ls = SA[0]; ll = (uint32_t)a.r; }
    else { ls = SA[i - 1]; ll = (uint32_t)a.l; }
    if (lane_id() == 0) {
        if (contains) contains[q] = (uint8_t)(j > i);
        if (range_lo) range_lo[q] = (uint32_t)i;
        if (range_hi) range_hi[q] = (uint32_t)j;
        if (lcp_start) lcp_start[q] = ls;
        if (lcp_len) lcp_len[q] = ll;
        if (stats) {
            atomicAdd(&stats[0], (unsigned long long)bytes);
            atomicAdd(&stats[1], (unsigned long long)(2 * log_p));
            atomicAdd(&stats[2], (unsigned long long)table_steps);
        }
    }
}

}  // namespace sa
