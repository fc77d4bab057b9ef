// kernels/docs.hpp -- document collections over the device index: positions to document ids
// (k_doc_of), the per-slot "previous slot of the same document" word (k_doc_prev), the units of a batch of match ranges
// (k_doc_ranges + the 64-bit exclusive scan), document frequency (k_doc_count) and document listing (k_doc_emit).
// gfx950, wave64.  Every index that is read is bounded by the table sizes passed in, whatever the arrays hold.
#pragma once
#include "common.hpp"

namespace sa {

constexpr uint32_t DOC_NONE = 0xffffffffu;
constexpr int DOC_SAMPLES = 8192;          // entries of the sampled top level of doc_off that every workgroup of k_doc_of stages (32 KiB of LDS)
constexpr int DOC_THREADS = 256;
constexpr int DOC_ITEMS = 8;               // positions per thread and trip of k_doc_of
constexpr int DOC_CHUNK_DEFAULT = 4096;    // slots of a unit (sa_amd_docs_set_chunk)
constexpr int DOC_CHUNK_MIN = 64;          // one coalesced load of a wave
constexpr int DOC_LOADS = 4;               // loads of the per-slot word a lane of k_doc_count has in flight
constexpr int DOC_CHUNK_MAX = 1 << 20;
constexpr int DOC_SCAN_THREADS = 256;
constexpr int DOC_SCAN_ITEMS = 8;
constexpr int DOC_SCAN_TILE = DOC_SCAN_THREADS * DOC_SCAN_ITEMS;
constexpr int DOC_SPINE_THREADS = 1024;

// doc(p) by a binary search of the whole table: the number of entries <= p, less one.  off: M = ndocs + 1 entries, off[0] = 0,
// off[M - 1] = n.  p >= n: DOC_NONE.
__device__ __forceinline__ uint32_t doc_lookup(const uint32_t *__restrict__ off, uint32_t M, uint32_t n, uint32_t p)
{
    if (p >= n) return DOC_NONE;
    uint32_t lo = 1, hi = M;                                  // first j in [1, M) with off[j] > p (off[M - 1] = n > p: it exists)
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (off[m] <= p) lo = m + 1; else hi = m;
    }
    return lo - 1;
}

// The sampled top level of the table: smp[k] = off[k * stride] for k < ns <= DOC_SAMPLES, staged by the whole workgroup
// (THREADS threads); ends in a barrier.
template <int THREADS>
__device__ __forceinline__ void doc_stage_samples(uint32_t *__restrict__ smp, const uint32_t *__restrict__ off, uint32_t M, uint32_t stride,
                                                  uint32_t ns, uint32_t n)
{
    for (uint32_t k = threadIdx.x; k < ns; k += THREADS) {
        const uint64_t j = (uint64_t)k * stride;
        smp[k] = j < M ? off[j] : n;
    }
    __syncthreads();
}

// doc(p) through the staged samples: the sample interval in LDS, then between two samples in the global table (at most
// ceil(log2 stride) loads).  p >= n: DOC_NONE.
__device__ __forceinline__ uint32_t doc_lookup_sampled(const uint32_t *__restrict__ smp, uint32_t ns, uint32_t stride,
                                                       const uint32_t *__restrict__ off, uint32_t M, uint32_t n, uint32_t p)
{
    if (p >= n) return DOC_NONE;
    uint32_t lo = 1, hi = ns;                                 // first k in [1, ns) with smp[k] > p, else ns
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (smp[m] <= p) lo = m + 1; else hi = m;
    }
    const uint64_t k0 = (uint64_t)(lo - 1) * stride;          // off[k0] <= p; off[k0 + stride] > p where it exists
    uint64_t e = k0 + stride;
    if (e > M) e = M;
    uint32_t a = (uint32_t)k0 + 1, b = (uint32_t)e;           // first j in [k0 + 1, e) with off[j] > p, else e
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (off[m] <= p) a = m + 1; else b = m;
    }
    return a - 1;
}

// pos[0 .. count) -> doc ids.  The workgroup stages off[0], off[s], off[2 s], ... (ns <= DOC_SAMPLES entries, s = stride) in LDS;
// a lane finds its sample interval there and finishes between two samples in the global table (at most ceil(log2 s) loads).
__global__ __launch_bounds__(DOC_THREADS) void k_doc_of(const uint32_t *__restrict__ pos, int64_t count, const uint32_t *__restrict__ off,
                                                       uint32_t M, uint32_t stride, uint32_t ns, uint32_t n, uint32_t *__restrict__ out)
{
    __shared__ uint32_t smp[DOC_SAMPLES];
    doc_stage_samples<DOC_THREADS>(smp, off, M, stride, ns, n);
    const int64_t span = (int64_t)DOC_THREADS * DOC_ITEMS;
    for (int64_t base = (int64_t)blockIdx.x * span; base < count; base += (int64_t)gridDim.x * span) {
        uint32_t p[DOC_ITEMS];
#pragma unroll
        for (int t = 0; t < DOC_ITEMS; ++t) {
            const int64_t i = base + (int64_t)t * DOC_THREADS + threadIdx.x;
            p[t] = i < count ? pos[i] : DOC_NONE;
        }
#pragma unroll
        for (int t = 0; t < DOC_ITEMS; ++t) {
            const int64_t i = base + (int64_t)t * DOC_THREADS + threadIdx.x;
            if (i >= count) continue;
            out[i] = doc_lookup_sampled(smp, ns, stride, off, M, n, p[t]);
        }
    }
}

// keys: the document ids of slots 1 .. n in stable order of the id, vals: their slot less one (nullptr: the order is that of
// the slots -- one document, nothing was sorted).  prev[slot] = previous slot of the same document + 1, 0 where there is none;
// prev[0] = 0xffffffff (the empty suffix belongs to no document and is never "first").
__global__ __launch_bounds__(DOC_THREADS) void k_doc_prev(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n,
                                                         uint32_t *__restrict__ prev)
{
    for (int64_t j = (int64_t)blockIdx.x * DOC_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * DOC_THREADS) {
        const uint32_t v = vals ? vals[j] : (uint32_t)j;
        if ((int64_t)v >= n) continue;                        // (cannot happen with a sound sort; never a store outside prev)
        uint32_t w = 0;
        if (j > 0 && keys[j - 1] == keys[j]) w = (vals ? vals[j - 1] : (uint32_t)(j - 1)) + 2;      // (slot = value + 1, stored + 1)
        prev[(int64_t)v + 1] = w;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) prev[0] = 0xffffffffu;
}

// ---- the units of a batch of ranges ----

// lo / hi as the search kernels left them -> lo (clamped), occ = hi - lo, units[q] = ceil(occ / chunk) for the scan (units[count] = 0:
// its scanned value is the number of all units).  ctl[1] += occ, ctl[2] += min(occ, ndocs) (the bound of the listing).
__global__ __launch_bounds__(DOC_THREADS) void k_doc_ranges(uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, int32_t count, uint32_t N1,
                                                           uint32_t chunk, uint32_t ndocs, uint32_t *__restrict__ occ,
                                                           unsigned long long *__restrict__ units, unsigned long long *__restrict__ ctl)
{
    const int64_t q = (int64_t)blockIdx.x * DOC_THREADS + threadIdx.x;
    if (q > count) return;
    if (q == count) { units[q] = 0; return; }
    uint32_t h = hi[q], l = lo[q];
    if (h > N1) h = N1;
    if (l > h) l = h;
    const uint32_t c = h - l;
    lo[q] = l;
    occ[q] = c;
    units[q] = ((unsigned long long)c + chunk - 1) / chunk;
    if (c) { atomicAdd(&ctl[1], (unsigned long long)c); atomicAdd(&ctl[2], (unsigned long long)(c < ndocs ? c : ndocs)); }
}

// ---- exclusive scan of uint64 words in place: tile sums, one workgroup over the tile sums, tiles again ----

__device__ __forceinline__ unsigned long long wave_incl_sum64(unsigned long long v)
{
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o, WAVE);
        if (l >= o) v += t;
    }
    return v;
}

template <int THREADS>
__device__ __forceinline__ unsigned long long block_excl_sum64(unsigned long long v, unsigned long long *lds, unsigned long long *total)
{
    constexpr int NW = THREADS / WAVE;
    const int l = lane_id(), w = wave_id();
    const unsigned long long inc = wave_incl_sum64(v);
    if (l == WAVE - 1) lds[w] = inc;
    __syncthreads();
    unsigned long long woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const unsigned long long s = lds[i];
        if (i < w) woff += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return woff + inc - v;
}

// PHASE 0: tsum[tile] = sum of the tile.  PHASE 1: v <- exclusive sums, tsum[tile] (scanned) the tile's base; the exclusive value of
// the LAST word goes to *last_out as well (nullptr: nowhere).  A thread owns DOC_SCAN_ITEMS consecutive words.
template <int PHASE>
__global__ __launch_bounds__(DOC_SCAN_THREADS) void k_doc_scan_tiles(unsigned long long *__restrict__ v, int64_t len, unsigned long long *__restrict__ tsum,
                                                                    unsigned long long *__restrict__ last_out)
{
    __shared__ unsigned long long lds[DOC_SCAN_THREADS / WAVE];
    const int64_t first = (int64_t)blockIdx.x * DOC_SCAN_TILE + (int64_t)threadIdx.x * DOC_SCAN_ITEMS;
    unsigned long long x[DOC_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int t = 0; t < DOC_SCAN_ITEMS; ++t) { x[t] = first + t < len ? v[first + t] : 0ull; s += x[t]; }
    unsigned long long tot;
    unsigned long long run = block_excl_sum64<DOC_SCAN_THREADS>(s, lds, &tot);
    if (PHASE == 0) { if (threadIdx.x == 0) tsum[blockIdx.x] = tot; return; }
    run += tsum[blockIdx.x];
#pragma unroll
    for (int t = 0; t < DOC_SCAN_ITEMS; ++t) {
        if (first + t < len) {
            v[first + t] = run;
            if (last_out && first + t == len - 1) *last_out = run;
        }
        run += x[t];
    }
}

// exclusive scan of tsum[0 .. tiles) in place by one workgroup: a thread owns a run of consecutive words
__global__ __launch_bounds__(DOC_SPINE_THREADS) void k_doc_scan_spine(unsigned long long *__restrict__ tsum, int64_t tiles)
{
    __shared__ unsigned long long lds[DOC_SPINE_THREADS / WAVE];
    const int64_t per = (tiles + DOC_SPINE_THREADS - 1) / DOC_SPINE_THREADS;
    const int64_t a = (int64_t)threadIdx.x * per, b = a + per < tiles ? a + per : tiles;
    unsigned long long s = 0;
    for (int64_t i = a; i < b; ++i) s += tsum[i];
    unsigned long long tot;
    unsigned long long run = block_excl_sum64<DOC_SPINE_THREADS>(s, lds, &tot);
    for (int64_t i = a; i < b; ++i) { const unsigned long long x = tsum[i]; tsum[i] = run; run += x; }
}

// ---- document frequency and listing: one wave per unit ----

// the pattern of unit u: the last q with uoff[q] <= u (uoff: count + 1 scanned words, uoff[count] = all units > u)
__device__ __forceinline__ uint32_t doc_unit_pattern(const unsigned long long *__restrict__ uoff, int32_t count, unsigned long long u)
{
    uint32_t lo = 1, hi = (uint32_t)count;                    // first q in [1, count) with uoff[q] > u, else count
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (uoff[m] <= u) lo = m + 1; else hi = m;
    }
    return lo - 1;
}

// the flagged slots of unit u of pattern q: those of [s0, s1) whose previous slot of the same document lies in front of the
// pattern's range -- one compare of the per-slot word against the range's left end.
// LIST = false: df[q] += the unit's count (integer atomics: the sum does not depend on the order).
// LIST = true: ucnt[u] = the count, uq[u] = q (k_doc_emit reads both).
template <bool LIST>
__global__ __launch_bounds__(DOC_THREADS) void k_doc_count(const uint32_t *__restrict__ prev, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ occ,
                                                          const unsigned long long *__restrict__ uoff, int32_t count, unsigned long long units,
                                                          uint32_t chunk, uint32_t *__restrict__ df, unsigned long long *__restrict__ ucnt,
                                                          uint32_t *__restrict__ uq)
{
    const int l = lane_id();
    const unsigned long long waves = (unsigned long long)gridDim.x * (DOC_THREADS / WAVE);
    for (unsigned long long u = (unsigned long long)blockIdx.x * (DOC_THREADS / WAVE) + wave_id(); u < units; u += waves) {
        const uint32_t q = doc_unit_pattern(uoff, count, u);
        const uint64_t k = u - uoff[q];
        const uint32_t l0 = lo[q], c = occ[q];
        const uint64_t r0 = k * chunk;
        uint32_t cnt = 0;
        if (r0 < c) {                                         // (always, for sound tables)
            const uint64_t r1 = r0 + chunk < c ? r0 + chunk : c;
            for (uint64_t r = r0; r < r1; r += DOC_LOADS * WAVE) {
                uint32_t w[DOC_LOADS];
#pragma unroll
                for (int t = 0; t < DOC_LOADS; ++t) {
                    const uint64_t i = r + (uint64_t)t * WAVE + l;
                    w[t] = i < r1 ? prev[l0 + i] : 0xffffffffu;      // (never <= l0: l0 <= n + 1 < 2^32 - 1)
                }
#pragma unroll
                for (int t = 0; t < DOC_LOADS; ++t) cnt += (uint32_t)__popcll(__ballot(w[t] <= l0));
            }
        }
        if (l == 0) {
            if (LIST) { ucnt[u] = cnt; uq[u] = q; }
            else if (cnt) atomicAdd(&df[q], cnt);
        }
    }
}

// The listing: unit u writes doc(SA[i]) of its flagged slots, in slot order, from uscan[u] on, while the offset is below
// `capacity`.  Units are ordered by pattern and then by slot, so the offsets are those of the whole batch's listing.
__global__ __launch_bounds__(DOC_THREADS) void k_doc_emit(const uint32_t *__restrict__ prev, const uint32_t *__restrict__ SA, const uint32_t *__restrict__ lo,
                                                         const uint32_t *__restrict__ occ, const unsigned long long *__restrict__ uoff,
                                                         const uint32_t *__restrict__ uq, const unsigned long long *__restrict__ uscan,
                                                         unsigned long long units, int32_t count, uint32_t chunk, const uint32_t *__restrict__ off,
                                                         uint32_t M, uint32_t n, uint32_t *__restrict__ docs, unsigned long long capacity)
{
    const int l = lane_id();
    const unsigned long long waves = (unsigned long long)gridDim.x * (DOC_THREADS / WAVE);
    for (unsigned long long u = (unsigned long long)blockIdx.x * (DOC_THREADS / WAVE) + wave_id(); u < units; u += waves) {
        unsigned long long at = uscan[u];
        if (at >= capacity || uscan[u + 1] == at) continue;   // nothing of this unit is listed or fits (wave-uniform)
        const uint32_t q = uq[u];
        if (q >= (uint32_t)count) continue;
        const uint64_t k = u - uoff[q];
        const uint32_t l0 = lo[q], c = occ[q];
        const uint64_t r0 = k * chunk;
        if (r0 >= c) continue;
        const uint64_t r1 = r0 + chunk < c ? r0 + chunk : c;
        for (uint64_t r = r0; r < r1 && at < capacity; r += WAVE) {
            const uint64_t i = r + l;
            const bool f = i < r1 && prev[l0 + i] <= l0;
            const unsigned long long b = __ballot(f);
            const unsigned long long o = at + (unsigned long long)__popcll(b & ((1ull << l) - 1ull));
            if (f && o < capacity) docs[o] = doc_lookup(off, M, n, SA[l0 + i]);
            at += (unsigned long long)__popcll(b);
        }
    }
}

// list_off[q] = uscan[uoff[q]] for q = 0 .. count: the listing's offsets per pattern, list_off[count] the number of all entries
__global__ __launch_bounds__(DOC_THREADS) void k_doc_list_off(const unsigned long long *__restrict__ uoff, const unsigned long long *__restrict__ uscan,
                                                             unsigned long long units, int32_t count, long long *__restrict__ list_off)
{
    const int64_t q = (int64_t)blockIdx.x * DOC_THREADS + threadIdx.x;
    if (q > count) return;
    unsigned long long u = uoff[q];
    if (u > units) u = units;
    list_off[q] = (long long)uscan[u];
}

}  // namespace sa
