// kernels/doc_tf.hpp -- per-document term frequencies and top-k documents over the device index: the
// slots ordered by document (k_doc_slots, the table behind sa_amd_index_enable_doc_freq), tf of every listed entry by two
// lower bounds in its document's part of that table (k_doc_tf), and the top-k of every pattern by a piecewise reduction:
// pieces of P keys sorted in LDS, the first k of each kept, until every pattern is one piece (k_topk_plan, k_topk_piece).
// gfx950, wave64.  Every index read through S, doc_off or the listing is bounded by the table sizes passed in, whatever the
// arrays hold.
#pragma once
#include "docs.hpp"

namespace sa {

constexpr int DOC_TOPK_MAX = 1024;             // SA_AMD_DOC_TOPK_MAX
constexpr int DOC_TOPK_PIECE_MIN = 64;         // keys of a piece (sa_amd_docs_set_topk_piece): a power of two
constexpr int DOC_TOPK_PIECE_MAX = 4096;       // 32 KiB of LDS
constexpr int DOC_TOPK_PIECE_DEFAULT = 1024;      // (level with 2048 and 4096, ahead on batches of many short listings)
constexpr int DOC_TOPK_THREADS = 256;

// vals: the slots less one in stable order of their document (nullptr: one document, the order of the slots).  S[j] = the slot.
__global__ __launch_bounds__(DOC_THREADS) void k_doc_slots(const uint32_t *__restrict__ vals, int64_t n, uint32_t *__restrict__ S)
{
    for (int64_t j = (int64_t)blockIdx.x * DOC_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * DOC_THREADS)
        S[j] = (vals ? vals[j] : (uint32_t)j) + 1u;
}

// One lane per listed entry e < entries: its pattern q is the last one with list_off[q] <= e, its document d = docs[e] owns
// S[off[d] .. off[d + 1]) (ascending slots), and tf = lb(hi) - lb(lo) with lb the lower bound in that part and [lo, hi) the
// pattern's range.  lb(lo) is a binary search of the part (where it holds the entry's flagged slot); lb(hi) gallops from there
// (GALLOP: probes at distance 1, 2, 4, ... and a binary search of the last gap -- O(log tf) loads) or is a second binary
// search of what is left of the part.  tf (nullptr: not wanted) and / or the reduction's key ((0xffffffff - tf) << 32) | d
// are written; ctl[3] += loads of S, ctl[4] += tf (one atomic per wave each).  d >= ndocs (an array that is no suffix array): tf = 0.
template <bool GALLOP>
__global__ __launch_bounds__(DOC_THREADS) void k_doc_tf(const uint32_t *__restrict__ S, const uint32_t *__restrict__ off, uint32_t ndocs, uint32_t n,
                                                       const uint32_t *__restrict__ lo, const uint32_t *__restrict__ occ,
                                                       const long long *__restrict__ list_off, int32_t count, const uint32_t *__restrict__ docs,
                                                       int64_t entries, uint32_t *__restrict__ tf, unsigned long long *__restrict__ keys,
                                                       unsigned long long *__restrict__ ctl)
{
    unsigned long long loads = 0, sum = 0;
    for (int64_t e = (int64_t)blockIdx.x * DOC_THREADS + threadIdx.x; e < entries; e += (int64_t)gridDim.x * DOC_THREADS) {
        uint32_t a = 1, b = (uint32_t)count;                  // first q in [1, count) with list_off[q] > e, else count
        while (a < b) {
            const uint32_t m = a + (b - a) / 2;
            if (list_off[m] <= e) a = m + 1; else b = m;
        }
        const uint32_t q = a - 1, d = docs[e];
        uint32_t f = 0;
        if (d < ndocs) {
            uint32_t s1 = off[d + 1], s0 = off[d];
            if (s1 > n) s1 = n;                               // (S has n entries)
            if (s0 > s1) s0 = s1;
            const uint32_t l0 = lo[q], h = l0 + occ[q];       // (k_doc_ranges: l0 + occ <= n + 1)
            uint32_t x = s0, y = s1;                          // first j in [s0, s1) with S[j] >= l0, else s1
            while (x < y) {
                const uint32_t m = x + (y - x) / 2;
                ++loads;
                if (S[m] < l0) x = m + 1; else y = m;
            }
            const uint32_t p0 = x;
            y = s1;                                           // first j in [p0, s1) with S[j] >= h, else s1
            if (GALLOP) {
                for (uint32_t step = 1;; step <<= 1) {        // (x + step - 1 < 2^31 + 2^31: step never exceeds the part)
                    const uint32_t probe = x + step - 1;
                    if (probe >= y) break;
                    ++loads;
                    if (S[probe] < h) x = probe + 1; else { y = probe; break; }
                }
            }
            while (x < y) {
                const uint32_t m = x + (y - x) / 2;
                ++loads;
                if (S[m] < h) x = m + 1; else y = m;
            }
            f = x - p0;
        }
        if (tf) tf[e] = f;
        if (keys) keys[e] = ((unsigned long long)(0xffffffffu - f) << 32) | d;
        sum += f;
    }
    loads = wave_incl_sum64(loads);
    sum = wave_incl_sum64(sum);
    if (lane_id() == WAVE - 1) {
        if (loads) atomicAdd(&ctl[3], loads);
        if (sum) atomicAdd(&ctl[4], sum);
    }
}

// ---- top-k by piecewise reduction ----

// A round's plan.  in_off: count + 1 offsets of the patterns' key lists.  pieces[q] = ceil(len / P) and outs[q] = what the
// pieces keep -- k of every full piece (k <= P / 2) and min(k, size) of the last -- for the scans; entry `count` of both is 0,
// so its scanned value is the sum.
__global__ __launch_bounds__(DOC_THREADS) void k_topk_plan(const unsigned long long *__restrict__ in_off, int32_t count, uint32_t P, uint32_t k,
                                                          unsigned long long *__restrict__ pieces, unsigned long long *__restrict__ outs)
{
    const int64_t q = (int64_t)blockIdx.x * DOC_THREADS + threadIdx.x;
    if (q > count) return;
    if (q == count) { pieces[q] = 0; outs[q] = 0; return; }
    const unsigned long long a = in_off[q], b = in_off[q + 1], len = b > a ? b - a : 0ull;
    const unsigned long long full = len / P, rest = len % P;
    pieces[q] = full + (rest ? 1 : 0);
    outs[q] = full * k + (rest < k ? rest : k);
}

// One workgroup per piece.  Piece p belongs to the last pattern q with poff[q] <= p and is its piece j = p - poff[q]: the keys
// in[in_off[q] + j P .. + size), size <= P.  They are staged in LDS, padded with all-ones to the next power of two, sorted
// ascending (bitonic) and the first min(k, size) go to the pattern's compact candidate list at ooff[q] + j k.  With docs / tf
// (the last round: every pattern is one piece) the keys are taken apart instead: the document below, 0xffffffff - tf above.
// in_total / out_total bound every index whatever the offsets hold.  Dynamic LDS: lds_keys * 8 bytes, lds_keys a power of two
// >= every piece of the round.
__global__ __launch_bounds__(DOC_TOPK_THREADS) void k_topk_piece(const unsigned long long *__restrict__ in, const unsigned long long *__restrict__ in_off,
                                                                unsigned long long in_total, const unsigned long long *__restrict__ poff,
                                                                const unsigned long long *__restrict__ ooff, int32_t count, uint32_t P, uint32_t k,
                                                                uint32_t lds_keys, unsigned long long *__restrict__ out, uint32_t *__restrict__ docs,
                                                                uint32_t *__restrict__ tf, unsigned long long out_total)
{
    extern __shared__ __align__(16) unsigned long long piece_keys[];
    const unsigned long long p = blockIdx.x;
    const uint32_t q = doc_unit_pattern(poff, count, p);
    const unsigned long long j = p - poff[q], a = in_off[q], b = in_off[q + 1] < in_total ? in_off[q + 1] : in_total;
    const unsigned long long r0 = a + j * P;
    if (p < poff[q] || r0 >= b) return;                       // (never, for sound offsets; uniform over the workgroup)
    const uint32_t size = (uint32_t)(b - r0 < P ? b - r0 : P);
    uint32_t m = 2;
    while (m < size) m <<= 1;
    if (m > lds_keys) return;                                 // (never: the host sized the LDS by the round's longest piece)
    for (uint32_t i = threadIdx.x; i < m; i += DOC_TOPK_THREADS) piece_keys[i] = i < size ? in[r0 + i] : ~0ull;
    __syncthreads();
    for (uint32_t kk = 2; kk <= m; kk <<= 1)
        for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
            for (uint32_t t = threadIdx.x; t < m / 2; t += DOC_TOPK_THREADS) {
                const uint32_t i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), l = i | jj;
                const unsigned long long x = piece_keys[i], y = piece_keys[l];
                if ((x > y) == ((i & kk) == 0)) { piece_keys[i] = y; piece_keys[l] = x; }
            }
            __syncthreads();
        }
    const uint32_t keep = size < k ? size : k;
    const unsigned long long o0 = ooff[q] + j * k;
    for (uint32_t i = threadIdx.x; i < keep; i += DOC_TOPK_THREADS) {
        const unsigned long long o = o0 + i, key = piece_keys[i];
        if (o >= out_total) continue;
        if (out) out[o] = key;
        if (docs) docs[o] = (uint32_t)key;
        if (tf) tf[o] = 0xffffffffu - (uint32_t)(key >> 32);
    }
}

}  // namespace sa
