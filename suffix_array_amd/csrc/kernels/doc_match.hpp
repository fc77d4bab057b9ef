// kernels/doc_match.hpp -- Boolean document queries over the device index: one bitmap of documents per
// clause, marked from the match ranges by the per-slot word's one compare (k_dm_mark), then AND / NOT over the clauses of a
// query word by word (k_dm_combine) and the set bits written out as ascending document ids (k_dm_emit).
// gfx950, wave64.  Every index that is read or written is bounded by the sizes passed in, whatever the arrays hold.
#pragma once
#include "docs.hpp"

namespace sa {

constexpr int DM_THREADS = 256;
constexpr int DM_LANE_WORDS = 4;                          // consecutive bitmap words of a lane: one 16-byte load per clause
constexpr int DM_TILE_WORDS = WAVE * DM_LANE_WORDS;       // words of a tile: what one wave combines (8 192 documents)

// A bitmap row has `stride` words, a multiple of DM_LANE_WORDS, of which the first W = ceil(ndocs / 32) carry documents: the
// words from W on are never marked, and the mask below clears them (and the bits from ndocs on in word W - 1) after a NOT.
__device__ __forceinline__ uint32_t dm_word_mask(uint64_t w, uint32_t W, uint32_t ndocs)
{
    if (w >= W) return 0u;
    if (w == (uint64_t)W - 1 && (ndocs & 31u)) return (1u << (ndocs & 31u)) - 1u;
    return 0xffffffffu;
}

__device__ __forceinline__ uint32_t dm_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// The marks of one slab: the units of the patterns [p0, p1) are uoff[p0] .. uoff[p1]; one wave per unit, with k_doc_emit's
// traversal of the per-slot word and DOC_LOADS loads of it in flight per lane.  A slot whose previous slot of the same document
// lies in front of the range is the first of its document there: it alone looks its document up -- through k_doc_of's samples of
// the offset table, staged in LDS by the workgroup (sstride, ns as launch_doc_of computes them) -- and sets the bit of its
// pattern's clause, so a call issues sum |D(p)| atomics, not sum occ.  Integer OR: the bitmap does not depend on the order.
// bits: (c1 - c0) rows of `stride` words, zeroed by the caller; marks (nullptr: not counted) += the slots that set a bit.
__global__ __launch_bounds__(DM_THREADS) void k_dm_mark(const uint32_t *__restrict__ prev, const uint32_t *__restrict__ SA, const uint32_t *__restrict__ lo,
                                                       const uint32_t *__restrict__ occ, const unsigned long long *__restrict__ uoff,
                                                       const uint32_t *__restrict__ pcl, int32_t count, unsigned long long units, uint32_t p0,
                                                       uint32_t p1, uint32_t c0, uint32_t c1, uint32_t chunk, const uint32_t *__restrict__ off,
                                                       uint32_t M, uint32_t sstride, uint32_t ns, uint32_t n, uint32_t stride,
                                                       uint32_t *__restrict__ bits, unsigned long long *__restrict__ marks)
{
    __shared__ uint32_t smp[DOC_SAMPLES];
    doc_stage_samples<DM_THREADS>(smp, off, M, sstride, ns, n);
    const int l = lane_id();
    const unsigned long long waves = (unsigned long long)gridDim.x * (DM_THREADS / WAVE);
    unsigned long long u1 = uoff[p1];                         // (p0 <= p1 <= count: uoff has count + 1 words)
    if (u1 > units) u1 = units;
    uint32_t made = 0;
    for (unsigned long long u = uoff[p0] + (unsigned long long)blockIdx.x * (DM_THREADS / WAVE) + wave_id(); u < u1; u += waves) {
        const uint32_t q = doc_unit_pattern(uoff, count, u);
        const uint32_t c = pcl[q];
        if (c < c0 || c >= c1) continue;                      // (never, for sound tables; never a store outside the slab)
        const uint64_t k = u - uoff[q];
        const uint32_t l0 = lo[q], cq = occ[q];
        const uint64_t r0 = k * chunk;
        if (r0 >= cq) continue;
        const uint64_t r1 = r0 + chunk < cq ? r0 + chunk : cq;
        uint32_t *__restrict__ row = bits + (size_t)(c - c0) * stride;
        for (uint64_t r = r0; r < r1; r += DOC_LOADS * WAVE) {
            uint32_t w[DOC_LOADS];
#pragma unroll
            for (int t = 0; t < DOC_LOADS; ++t) {
                const uint64_t i = r + (uint64_t)t * WAVE + l;
                w[t] = i < r1 ? prev[l0 + i] : 0xffffffffu;          // (never <= l0: l0 <= n + 1 < 2^32 - 1)
            }
#pragma unroll
            for (int t = 0; t < DOC_LOADS; ++t) {
                if (w[t] <= l0) {
                    const uint32_t d = doc_lookup_sampled(smp, ns, sstride, off, M, n, SA[l0 + r + (uint64_t)t * WAVE + l]);
                    if (d < M - 1) {                          // (DOC_NONE only for an array that is no suffix array)
                        atomicOr(&row[d >> 5], 1u << (d & 31u));
                        ++made;
                    }
                }
            }
        }
    }
    if (marks) {
        made = dm_wave_sum(made);
        if (l == 0 && made) atomicAdd(marks, (unsigned long long)made);
    }
}

// the words [w0, w0 + DM_LANE_WORDS) of query words: all ones, ANDed with every clause's row (complemented where the clause is
// negated), then masked -- a query without clauses keeps every document and nothing beyond them.  With CDF the masked
// popcount of every clause's own set goes to clause_df: a clause belongs to one query, so its words pass here exactly once.
template <bool CDF>
__device__ __forceinline__ void dm_query_words(const uint32_t *__restrict__ bits, const uint8_t *__restrict__ cflags, uint32_t ca, uint32_t cb,
                                               uint32_t c0, uint32_t stride, uint32_t W, uint32_t ndocs, uint64_t w0,
                                               uint32_t *__restrict__ clause_df, uint32_t acc[DM_LANE_WORDS])
{
    uint32_t mask[DM_LANE_WORDS];
#pragma unroll
    for (int t = 0; t < DM_LANE_WORDS; ++t) { mask[t] = dm_word_mask(w0 + t, W, ndocs); acc[t] = 0xffffffffu; }
    const bool in = w0 < stride;                              // (stride is a multiple of DM_LANE_WORDS: all four words or none)
    for (uint32_t c = ca; c < cb; ++c) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (in) v = *reinterpret_cast<const uint4 *>(bits + (size_t)(c - c0) * stride + w0);
        const uint32_t neg = (cflags[c] & 1u) ? 0xffffffffu : 0u;
        const uint32_t x[DM_LANE_WORDS] = { v.x ^ neg, v.y ^ neg, v.z ^ neg, v.w ^ neg };
        if (CDF) {
            uint32_t cnt = 0;
#pragma unroll
            for (int t = 0; t < DM_LANE_WORDS; ++t) cnt += (uint32_t)__popc(x[t] & mask[t]);
            cnt = dm_wave_sum(cnt);
            if (lane_id() == 0 && cnt) atomicAdd(&clause_df[c], cnt);
        }
#pragma unroll
        for (int t = 0; t < DM_LANE_WORDS; ++t) acc[t] &= x[t];
    }
#pragma unroll
    for (int t = 0; t < DM_LANE_WORDS; ++t) acc[t] &= mask[t];
}

// One wave per (query of the slab, tile of words).  LIST = false: df[q] += the tile's documents (one integer atomic a wave).
// LIST = true: tcnt[q * tiles + tile] = that number, for the scan that gives every tile its place in the listing.
// qoff: the clauses of query q are [qoff[q], qoff[q + 1]), all inside the slab's [c0, c1).
template <bool LIST, bool CDF>
__global__ __launch_bounds__(DM_THREADS) void k_dm_combine(const uint32_t *__restrict__ bits, const int32_t *__restrict__ qoff,
                                                          const uint8_t *__restrict__ cflags, uint32_t q0, uint32_t q1, uint32_t c0, uint32_t c1,
                                                          uint32_t stride, uint32_t W, uint32_t ndocs, uint32_t tiles, uint32_t *__restrict__ df,
                                                          uint32_t *__restrict__ clause_df, unsigned long long *__restrict__ tcnt)
{
    const int l = lane_id();
    const unsigned long long items = (unsigned long long)(q1 - q0) * tiles, waves = (unsigned long long)gridDim.x * (DM_THREADS / WAVE);
    for (unsigned long long it = (unsigned long long)blockIdx.x * (DM_THREADS / WAVE) + wave_id(); it < items; it += waves) {
        const uint32_t q = q0 + (uint32_t)(it / tiles), tile = (uint32_t)(it % tiles);
        uint32_t ca = (uint32_t)qoff[q], cb = (uint32_t)qoff[q + 1];
        if (ca < c0) ca = c0;                                 // (never, for the offsets the host checked)
        if (cb > c1) cb = c1;
        uint32_t acc[DM_LANE_WORDS];
        dm_query_words<CDF>(bits, cflags, ca, cb, c0, stride, W, ndocs, (uint64_t)tile * DM_TILE_WORDS + (uint64_t)l * DM_LANE_WORDS, clause_df, acc);
        uint32_t cnt = 0;
#pragma unroll
        for (int t = 0; t < DM_LANE_WORDS; ++t) cnt += (uint32_t)__popc(acc[t]);
        cnt = dm_wave_sum(cnt);
        if (l == 0) {
            if (LIST) tcnt[(unsigned long long)q * tiles + tile] = cnt;
            else if (cnt) atomicAdd(&df[q], cnt);
        }
    }
}

// The listing: the wave of (query, tile) computes its words again, ranks its lanes by a prefix sum of their popcounts and
// writes the document id of every set bit, ascending, from tscan[q * tiles + tile] on while the offset is below `capacity`.
// A lane owns consecutive words and tiles are scanned in the order of query and tile, so each query's listing ascends.
__global__ __launch_bounds__(DM_THREADS) void k_dm_emit(const uint32_t *__restrict__ bits, const int32_t *__restrict__ qoff, const uint8_t *__restrict__ cflags,
                                                       uint32_t q0, uint32_t q1, uint32_t c0, uint32_t c1, uint32_t stride, uint32_t W, uint32_t ndocs,
                                                       uint32_t tiles, const unsigned long long *__restrict__ tscan, uint32_t *__restrict__ docs,
                                                       unsigned long long capacity)
{
    const int l = lane_id();
    const unsigned long long items = (unsigned long long)(q1 - q0) * tiles, waves = (unsigned long long)gridDim.x * (DM_THREADS / WAVE);
    for (unsigned long long it = (unsigned long long)blockIdx.x * (DM_THREADS / WAVE) + wave_id(); it < items; it += waves) {
        const uint32_t q = q0 + (uint32_t)(it / tiles), tile = (uint32_t)(it % tiles);
        const unsigned long long at = tscan[(unsigned long long)q * tiles + tile];
        if (at >= capacity || tscan[(unsigned long long)q * tiles + tile + 1] == at) continue;      // nothing of this tile is listed or fits (wave-uniform)
        uint32_t ca = (uint32_t)qoff[q], cb = (uint32_t)qoff[q + 1];
        if (ca < c0) ca = c0;
        if (cb > c1) cb = c1;
        const uint64_t w0 = (uint64_t)tile * DM_TILE_WORDS + (uint64_t)l * DM_LANE_WORDS;
        uint32_t acc[DM_LANE_WORDS];
        dm_query_words<false>(bits, cflags, ca, cb, c0, stride, W, ndocs, w0, nullptr, acc);
        uint32_t cnt = 0;
#pragma unroll
        for (int t = 0; t < DM_LANE_WORDS; ++t) cnt += (uint32_t)__popc(acc[t]);
        unsigned long long o = at + (wave_incl_sum(cnt) - cnt);
#pragma unroll
        for (int t = 0; t < DM_LANE_WORDS; ++t) {
            uint32_t x = acc[t];
            while (x) {
                const uint32_t b = (uint32_t)__ffs((int)x) - 1u;
                if (o < capacity) docs[o] = (uint32_t)((w0 + t) << 5) + b;
                ++o;
                x &= x - 1u;
            }
        }
    }
}

// list_off[q] = tscan[q * tiles] for q = 0 .. nqueries (tscan has nqueries * tiles + 1 scanned words: the last is the total)
__global__ __launch_bounds__(DM_THREADS) void k_dm_list_off(const unsigned long long *__restrict__ tscan, uint32_t tiles, int32_t nqueries,
                                                           long long *__restrict__ list_off)
{
    const int64_t q = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    if (q > nqueries) return;
    list_off[q] = (long long)tscan[(unsigned long long)q * tiles];
}

}  // namespace sa
