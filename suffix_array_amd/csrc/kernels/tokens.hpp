// kernels/tokens.hpp -- texts over a token alphabet: 16-bit tokens and token ids below 2^24 in 32-bit
// storage (section 25).  Construction: the big-endian byte image B of the token text, STRIDE = 2 or 3 bytes a token
// (k_tok_be_image, k_tok_be_image3), the byte builder on B, then an order-preserving compaction that keeps the entries of B's
// suffix array that are divisible by STRIDE, divided by it (k_tok_compact_count, one scan, k_tok_compact_scatter) -- big-endian
// bytes compare like the tokens and two suffixes of B at offsets divisible by STRIDE have lengths divisible by STRIDE, so their
// byte order is the token order.  Queries over a resident token index, written once over Sym = uint16_t / uint32_t:
// range search (k_tok_search), back-off (k_infgram_suffix<uint16_t>, <uint32_t>) and the counts of the token that follows a
// context (k_tok_next), the token forms of kernels/ngram.hpp.  One wave per query, no atomics on the answers.  Documents from a
// separator token (section 27): the compaction's shape over the text itself (k_tok_sep_count, one scan, k_tok_sep_emit).
// gfx950, wave64.
// Every slot read lies in [0, n + 1) and every SA entry is checked against n before T is read through it, whatever the arrays hold.
#pragma once
#include "ngram.hpp"

namespace sa {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / WAVE;
constexpr int TK_LOADS = 2;                                 // 16-byte loads a work-item of the compaction has in flight
constexpr int TK_CHUNK = WAVE * 4;                          // entries of one wave-wide 16-byte load
constexpr int TK_WAVE_ITEMS = TK_LOADS * TK_CHUNK;          // consecutive entries a wave owns in a tile
constexpr int TK_TILE = TK_WAVES * TK_WAVE_ITEMS;           // 2048 entries of the byte-level array: one count
constexpr int TK_SPAN = 4;                                  // consecutive tiles a workgroup takes in one trip
constexpr int TK_IMAGE_ITEMS = 8;                           // tokens per work-item of the image pass: one 16-byte load and store
constexpr int TK_IMAGE3_ITEMS = 16;                         // tokens per work-item of the 3-byte image pass: four 16-byte loads, three stores
constexpr int TK_END = 65536;                               // the "token" of a slot whose suffix ends at the context: sym_end<uint16_t>()
constexpr uint32_t TK_LIMIT_U32 = 1u << 24;                 // SA_AMD_TOKEN_LIMIT_U32: the ids of a 32-bit token text lie below it (= sym_end<uint32_t>())

// the bytes a token of Sym has in the image: the stride of the kept entries of the byte-level array
template <typename Sym> struct TokStrideOf;
template <> struct TokStrideOf<uint16_t> { static constexpr int value = 2; };
template <> struct TokStrideOf<uint32_t> { static constexpr int value = 3; };
template <int STRIDE> struct TokStride { };                 // a kernel argument: the compaction's stride is deduced from it

// B[2 i] = T[i] >> 8, B[2 i + 1] = T[i] & 255 for i < n: the two bytes of every token swapped.  T and B are 16-byte aligned and
// their slabs end at or behind the 16-byte group of the last token; the bytes of B behind 2 n are written as zeros.
__global__ __launch_bounds__(TK_THREADS) void k_tok_be_image(const uint16_t *__restrict__ T, uint8_t *__restrict__ B, int64_t n)
{
    const int64_t groups = (n + TK_IMAGE_ITEMS - 1) / TK_IMAGE_ITEMS;
    for (int64_t g = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * TK_THREADS) {
        const int64_t first = g * TK_IMAGE_ITEMS;
        uint4 v = *reinterpret_cast<const uint4 *>(T + first);
        uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t x = ((w[k] & 0x00ff00ffu) << 8) | ((w[k] >> 8) & 0x00ff00ffu);
            const int64_t left = n - (first + 2 * k);      // tokens of this word that exist
            if (left < 2) x = left == 1 ? (x & 0xffffu) : 0u;
            w[k] = x;
        }
        *reinterpret_cast<uint4 *>(B + 2 * first) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The 3-byte image: B[3 i] = T[i] >> 16, B[3 i + 1] = (T[i] >> 8) & 255, B[3 i + 2] = T[i] & 255 for i < n.  A work-item takes 16
// tokens: four 16-byte loads (one that starts at or behind token n is not made), twelve words, three aligned 16-byte stores (one
// that starts at or behind byte 3 n is not made); the bytes of B behind 3 n in the last store are zeros.  T and B are 16-byte
// aligned with 16 bytes of slack behind the tokens / the image.  flags[0] |= 1 where a token is not below 2^24 (its low 24 bits
// go to the image): one ballot and one atomic per wave, as k_tok_sa_range.
__global__ __launch_bounds__(TK_THREADS) void k_tok_be_image3(const uint32_t *__restrict__ T, uint8_t *__restrict__ B, int64_t n,
                                                             uint32_t *__restrict__ flags)
{
    const int64_t groups = (n + TK_IMAGE3_ITEMS - 1) / TK_IMAGE3_ITEMS;
    bool bad = false;
    for (int64_t g = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * TK_THREADS) {
        const int64_t first = g * TK_IMAGE3_ITEMS;
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = first + 4 * k < n ? *reinterpret_cast<const uint4 *>(T + first + 4 * k) : make_uint4(0u, 0u, 0u, 0u);
        uint32_t w[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t t[4] = { v[k].x, v[k].y, v[k].z, v[k].w }, p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (first + 4 * k + i >= n) t[i] = 0u;                     // (slack behind the text: any bytes)
                bad |= t[i] >= TK_LIMIT_U32;
                p[i] = __builtin_bswap32(t[i]) >> 8;                       // the token's three bytes, the top one lowest
            }
            w[3 * k] = p[0] | (p[1] << 24);
            w[3 * k + 1] = (p[1] >> 8) | (p[2] << 16);
            w[3 * k + 2] = (p[2] >> 16) | (p[3] << 8);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (3 * first + 16 * k < 3 * n)
                *reinterpret_cast<uint4 *>(B + 3 * first + 16 * k) = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
    if (__ballot(bad) && lane_id() == 0) atomicOr(flags, 1u);
}

// flags[0] |= 1 where a token of T[0 .. n) is not below 2^24: the range pass over a 32-bit token text that is not built from
__global__ __launch_bounds__(TK_THREADS) void k_tok_id_range(const uint32_t *__restrict__ T, int64_t n, uint32_t *__restrict__ flags)
{
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TK_THREADS)
        bad |= T[i] >= TK_LIMIT_U32;
    if (__ballot(bad) && lane_id() == 0) atomicOr(flags, 1u);
}

// Is the entry e of the byte-level array kept, and *q = e / STRIDE where it is.  STRIDE 2: the even entries, halved.  STRIDE 3:
// 0xAAAAAAAB is the inverse of 3 modulo 2^32, so e = 3 k gives e * 0xAAAAAAAB = k <= 0x55555555 = (2^32 - 1) / 3, and the
// products of the other residues lie above: one multiply is the test and the quotient.
template <int STRIDE>
__device__ __forceinline__ bool tok_kept(uint32_t e, uint32_t *q)
{
    static_assert(STRIDE == 2 || STRIDE == 3, "bytes of a token in the image");
    if constexpr (STRIDE == 2) { *q = e >> 1; return !(e & 1u); }
    else { *q = e * 0xAAAAAAABu; return *q <= 0x55555555u; }
}

// The entries [base, base + 4) of the byte-level array that a lane holds after one 16-byte load, and which of them are kept:
// bit k of the result is set iff base + k < len and the entry is divisible by STRIDE; e[k] = the entry divided by STRIDE then.
// The slab ends at or behind the 16-byte group of the last entry, so the load is in range wherever base < len.
template <int STRIDE>
__device__ __forceinline__ uint32_t tok_compact_load(const uint32_t *__restrict__ SA2, int64_t len, int64_t base, uint32_t e[4])
{
    uint32_t keep = 0;
    if (base < len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(SA2 + base);
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (tok_kept<STRIDE>(e[k], &e[k]) && base + k < len) keep |= 1u << k;
    }
    return keep;
}

// cnt[t] = the number of kept entries of tile t of SA2[0 .. len); cnt[tiles] = 0 (the scan leaves the number of all kept
// entries there).  A workgroup takes TK_SPAN tiles a trip, a wave TK_WAVE_ITEMS consecutive entries of each.
template <int STRIDE>
__global__ __launch_bounds__(TK_THREADS) void k_tok_compact_count(const uint32_t *__restrict__ SA2, int64_t len, int64_t tiles,
                                                                 unsigned long long *__restrict__ cnt, TokStride<STRIDE>)
{
    __shared__ uint32_t s_w[TK_SPAN][TK_WAVES];
    const int l = lane_id(), w = wave_id();
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[tiles] = 0ull;
    const int64_t spans = (tiles + TK_SPAN - 1) / TK_SPAN;
    for (int64_t sp = blockIdx.x; sp < spans; sp += gridDim.x) {
#pragma unroll
        for (int t = 0; t < TK_SPAN; ++t) {
            const int64_t tile = sp * TK_SPAN + t;
            uint32_t kept = 0;
#pragma unroll
            for (int c = 0; c < TK_LOADS; ++c) {
                uint32_t e[4];
                const int64_t base = tile * TK_TILE + (int64_t)w * TK_WAVE_ITEMS + c * TK_CHUNK + 4 * l;
                kept += (uint32_t)__popc(tok_compact_load<STRIDE>(SA2, len, base, e));
            }
            kept = wave_incl_sum(kept);
            if (l == WAVE - 1) s_w[t][w] = kept;
        }
        __syncthreads();
        if (threadIdx.x < TK_SPAN && sp * TK_SPAN + threadIdx.x < tiles) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < TK_WAVES; ++i) s += s_w[threadIdx.x][i];
            cnt[sp * TK_SPAN + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// out[off[t] + r] = SA2[i] / STRIDE for the r-th kept entry i of tile t, off the scanned counts: the kept entries in their order.
// The rank of an entry inside its wave comes from the ballots of the four components of a load and their popcounts below the
// lane; the waves of a tile meet in LDS.  Exactly off[tiles] <= out_len entries are written.
template <int STRIDE>
__global__ __launch_bounds__(TK_THREADS) void k_tok_compact_scatter(const uint32_t *__restrict__ SA2, int64_t len, int64_t tiles,
                                                                   const unsigned long long *__restrict__ off, uint32_t *__restrict__ out,
                                                                   int64_t out_len, TokStride<STRIDE>)
{
    __shared__ uint32_t s_w[TK_WAVES];
    const int l = lane_id(), w = wave_id();
    const uint64_t below = (1ull << l) - 1ull;
    const int64_t spans = (tiles + TK_SPAN - 1) / TK_SPAN;
    for (int64_t sp = blockIdx.x; sp < spans; sp += gridDim.x) {
        for (int t = 0; t < TK_SPAN; ++t) {
            const int64_t tile = sp * TK_SPAN + t;
            if (tile >= tiles) break;                                 // (the same for every work-item)
            uint32_t e[TK_LOADS][4], keep[TK_LOADS], rank[TK_LOADS], total = 0;
#pragma unroll
            for (int c = 0; c < TK_LOADS; ++c)
                keep[c] = tok_compact_load<STRIDE>(SA2, len, tile * TK_TILE + (int64_t)w * TK_WAVE_ITEMS + c * TK_CHUNK + 4 * l, e[c]);
#pragma unroll
            for (int c = 0; c < TK_LOADS; ++c) {
                uint32_t before = 0, all = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint64_t b = __ballot((keep[c] >> k) & 1u);
                    before += (uint32_t)__popcll(b & below);
                    all += (uint32_t)__popcll(b);
                }
                rank[c] = total + before;
                total += all;
            }
            if (l == 0) s_w[w] = total;
            __syncthreads();
            unsigned long long o = off[tile];
#pragma unroll
            for (int i = 0; i < TK_WAVES; ++i) if (i < w) o += s_w[i];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < TK_LOADS; ++c) {
                unsigned long long at = o + rank[c];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!((keep[c] >> k) & 1u)) continue;
                    if ((int64_t)at < out_len) out[at] = e[c][k];
                    ++at;
                }
            }
        }
    }
}

// flags[0] |= 1 where an entry of SA[0 .. n + 1) exceeds n: the range pass over a caller's array
__global__ __launch_bounds__(TK_THREADS) void k_tok_sa_range(const uint32_t *__restrict__ SA, int64_t n, uint32_t *__restrict__ flags)
{
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * TK_THREADS)
        bad |= (int64_t)SA[i] > n;
    if (__ballot(bad) && lane_id() == 0) atomicOr(flags, 1u);
}

// ---- documents from a separator token: the positions of `sep` in T[0 .. n), each plus one, in their
//      order -- the compaction above with the text for the byte-level array and "equals sep" for "divisible by STRIDE" ----

template <typename Sym> struct TokSepOf {
    static constexpr int PER = 16 / (int)sizeof(Sym);                   // tokens of one lane's 16-byte load: 8 or 4
    static constexpr int LOADS = TK_WAVE_ITEMS / (WAVE * PER);          // wave-wide loads that cover a wave's share of a tile: 1 or 2
    static_assert(LOADS * WAVE * PER == TK_WAVE_ITEMS, "whole loads cover a wave's share of a tile");
};

// The PER tokens [base, base + PER) that a lane holds after one 16-byte load: bit k of the result is set iff base + k < n and
// T[base + k] == sep.  T is 16-byte aligned with 16 bytes of slack behind the tokens and base is a multiple of PER, so the load
// is in range wherever base < n; what it brings from behind n is masked by index.
template <typename Sym>
__device__ __forceinline__ uint32_t tok_sep_load(const Sym *__restrict__ T, int64_t n, int64_t base, uint32_t sep)
{
    constexpr int PER = TokSepOf<Sym>::PER;
    uint32_t m = 0;
    if (base < n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(T + base);
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            uint32_t t;
            if constexpr (sizeof(Sym) == 2) t = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu; else t = w[k];
            if (t == sep && base + k < n) m |= 1u << k;
        }
    }
    return m;
}

// the flags of component k of a wave-wide load: how many lanes hold one, and how many of those lie below this lane
__device__ __forceinline__ void tok_sep_ballot(uint32_t m, int k, uint32_t *before, uint32_t *all)
{
    const uint64_t b = __ballot((m >> k) & 1u);
    *before += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    *all += (uint32_t)__popcll(b);
}

// cnt[t] = the number of separators in tile t (TK_TILE tokens) of T[0 .. n); cnt[tiles] = 0 (the scan leaves the number k of all
// separators there) and cnt[tiles + 1] = 1 iff a last document runs to n behind the last separator (n == 0 or T[n - 1] != sep),
// which the scan does not touch: the two words come back together.  A workgroup takes TK_SPAN tiles a trip, a wave
// TK_WAVE_ITEMS consecutive tokens of each; a tile's count is the popcounts of its waves' ballots, summed in LDS.
template <typename Sym>
__global__ __launch_bounds__(TK_THREADS) void k_tok_sep_count(const Sym *__restrict__ T, int64_t n, int64_t tiles, uint32_t sep,
                                                             unsigned long long *__restrict__ cnt)
{
    constexpr int PER = TokSepOf<Sym>::PER, LOADS = TokSepOf<Sym>::LOADS;
    __shared__ uint32_t s_w[TK_SPAN][TK_WAVES];
    const int l = lane_id(), w = wave_id();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt[tiles] = 0ull;
        cnt[tiles + 1] = n == 0 || (uint32_t)T[n - 1] != sep ? 1ull : 0ull;
    }
    const int64_t spans = (tiles + TK_SPAN - 1) / TK_SPAN;
    for (int64_t sp = blockIdx.x; sp < spans; sp += gridDim.x) {
#pragma unroll
        for (int t = 0; t < TK_SPAN; ++t) {
            const int64_t tile = sp * TK_SPAN + t;
            uint32_t m[LOADS], before = 0, all = 0;
#pragma unroll
            for (int c = 0; c < LOADS; ++c)
                m[c] = tok_sep_load(T, n, tile * TK_TILE + (int64_t)w * TK_WAVE_ITEMS + (int64_t)c * WAVE * PER + PER * l, sep);
#pragma unroll
            for (int c = 0; c < LOADS; ++c)
#pragma unroll
                for (int k = 0; k < PER; ++k) tok_sep_ballot(m[c], k, &before, &all);
            if (l == 0) s_w[t][w] = all;
        }
        __syncthreads();
        if (threadIdx.x < TK_SPAN && sp * TK_SPAN + threadIdx.x < tiles) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < TK_WAVES; ++i) s += s_w[threadIdx.x][i];
            cnt[sp * TK_SPAN + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// doc_off[1 + base[t] + r] = p + 1 for the r-th separator p of tile t, base the scanned counts: the ends of the documents in
// their order.  The flags are computed again; the rank of a lane's first separator inside its wave is mbcnt over the ballots of
// the PER components (the lanes below hold the tokens before its own), the waves of a tile meet in LDS.  One work-item writes
// doc_off[0] = 0 and, `closing`, doc_off[k + 1] = n.  Entries 1 .. k are written and no other, whatever base holds.
template <typename Sym>
__global__ __launch_bounds__(TK_THREADS) void k_tok_sep_emit(const Sym *__restrict__ T, int64_t n, int64_t tiles, uint32_t sep,
                                                            const unsigned long long *__restrict__ base, uint32_t *__restrict__ doc_off,
                                                            unsigned long long k_all, uint32_t closing)
{
    constexpr int PER = TokSepOf<Sym>::PER, LOADS = TokSepOf<Sym>::LOADS;
    __shared__ uint32_t s_w[TK_WAVES];
    const int l = lane_id(), w = wave_id();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        doc_off[0] = 0u;
        if (closing) doc_off[k_all + 1] = (uint32_t)n;
    }
    const int64_t spans = (tiles + TK_SPAN - 1) / TK_SPAN;
    for (int64_t sp = blockIdx.x; sp < spans; sp += gridDim.x) {
        for (int t = 0; t < TK_SPAN; ++t) {
            const int64_t tile = sp * TK_SPAN + t;
            if (tile >= tiles) break;                                 // (the same for every work-item)
            const int64_t first = tile * TK_TILE + (int64_t)w * TK_WAVE_ITEMS + PER * l;
            uint32_t m[LOADS], rank[LOADS], total = 0;
#pragma unroll
            for (int c = 0; c < LOADS; ++c) m[c] = tok_sep_load(T, n, first + (int64_t)c * WAVE * PER, sep);
#pragma unroll
            for (int c = 0; c < LOADS; ++c) {
                uint32_t before = 0, all = 0;
#pragma unroll
                for (int k = 0; k < PER; ++k) tok_sep_ballot(m[c], k, &before, &all);
                rank[c] = total + before;
                total += all;
            }
            if (l == 0) s_w[w] = total;
            __syncthreads();
            unsigned long long o = base[tile];
#pragma unroll
            for (int i = 0; i < TK_WAVES; ++i) if (i < w) o += s_w[i];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < LOADS; ++c) {
                unsigned long long at = o + rank[c];
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    if (!((m[c] >> k) & 1u)) continue;
                    if (at < k_all) doc_off[at + 1] = (uint32_t)(first + (int64_t)c * WAVE * PER + k + 1);
                    ++at;
                }
            }
        }
    }
}

// Range search of `count` patterns, one wave each (a wave takes every waves-th pattern): plain_range (kernels/sym.hpp) over the
// n + 1 slots, no bucket table and no LCP table; pat_off in tokens.  Every output may be nullptr.
template <typename Sym>
__global__ __launch_bounds__(NG_THREADS) void k_tok_search(
    const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const Sym *__restrict__ pat_data,
    const int64_t *__restrict__ pat_off, int32_t count, uint8_t *__restrict__ contains, uint32_t *__restrict__ range_lo,
    uint32_t *__restrict__ range_hi)
{
    const int64_t waves = (int64_t)gridDim.x * NG_WAVES;
    int64_t tokens = 0;
    for (int64_t q = (int64_t)blockIdx.x * NG_WAVES + wave_id(); q < count; q += waves) {
        const NgRange r = plain_range(T, SA, n, 0, n + 1, pat_data + pat_off[q], pat_off[q + 1] - pat_off[q], &tokens);
        if (lane_id() == 0) {
            if (contains) contains[q] = r.hi > r.lo ? 1 : 0;
            if (range_lo) range_lo[q] = r.lo;
            if (range_hi) range_hi[q] = r.hi;
        }
    }
}

// one entry of a listing: the token and count of the run with rank `r` behind the listing's offset `o`
template <typename Sym>
__device__ __forceinline__ void tok_emit_token(Sym *__restrict__ toks, unsigned long long o, uint32_t r, unsigned long long capacity, int tok)
{
    if (toks && o + r < capacity) toks[o + r] = (Sym)tok;
}
__device__ __forceinline__ void tok_emit_count(uint32_t *__restrict__ counts, unsigned long long o, uint32_t r, unsigned long long capacity, uint32_t c)
{
    if (counts && o + r < capacity) counts[o + r] = c;
}

// Continuations of query q over its window (ng_window of kernels/ngram.hpp: s0, cnt, p, at_end).  Inside the range the slots
// are sorted by the token behind the context, so the listing is the list of the runs of equal tokens: a run STARTS at place i
// (relative to s0) where the token differs from the one at i - 1, and its count is the next start (or cnt) less its own.  A run
// of TK_END = sym_end<Sym>() (only an array that is no suffix array has one behind s0) ends the run before it and is not listed.  There is no
// table per query: a run's rank in the listing is the number of listed starts before it.
//   cnt <= stream_cap: the range is read once, NG_LOADS * 64 slots a trip; a lane compares its token with its left neighbour's
//     (a shuffle; the last token of a trip is carried into the next).  The ranks come from the ballot of the listed starts, the
//     count of a start from the next set bit of the ballot of all starts; the last start of a ballot waits (wave-uniform
//     registers) for the first start of a later one.  cnt slots probed.
//   else: the 64 samples and the walk between them (ng_sample, ng_walk of kernels/ngram.hpp), walked once to count and, EMIT,
//     once more to emit; only the first walk's probes are counted.  At most 64 + D (ceil(log2(cnt + 1)) + 1) slots probed for D
//     distinct continuations.  A lane's ranks start at the exclusive sum of the starts the lanes before it found; the count of a
//     lane's last run ends at the first start of a later lane.
// EMIT = false: nnz[q] = the number of listed runs (nnz[count] is the host's), at_end[q], and the counters -- one atomic per
// wave each behind all of its queries.  EMIT = true: nnz holds the scanned offsets; the (token, count) pairs go to toks /
// counts (either may be nullptr) in ascending token order from nnz[q] on, while the offset is below `capacity`.
template <bool EMIT, typename Sym>
__global__ __launch_bounds__(NG_THREADS) void k_tok_next(
    const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ range_lo,
    const uint32_t *__restrict__ range_hi, const uint32_t *__restrict__ depth, const int64_t *__restrict__ pat_off, int32_t count,
    uint32_t stream_cap, uint8_t *__restrict__ at_end, unsigned long long *__restrict__ nnz, Sym *__restrict__ toks,
    uint32_t *__restrict__ counts, unsigned long long capacity, unsigned long long *__restrict__ ctl)
{
    constexpr int TK_END = sym_end<Sym>();
    const int l = lane_id();
    const uint64_t below = (1ull << l) - 1ull;
    const int64_t waves = (int64_t)gridDim.x * NG_WAVES;
    NgCounters ctr;
    for (int64_t q = (int64_t)blockIdx.x * NG_WAVES + wave_id(); q < count; q += waves) {
        const NgWindow w = ng_window(SA, n, range_lo, range_hi, depth, pat_off, q);
        const uint32_t cnt = w.cnt;
        const unsigned long long o = EMIT ? nnz[q] : 0ull;
        uint32_t listed = 0;                                              // listed runs so far (the same in every lane)
        if (cnt == 0) {
            ++ctr.empty_q;
        } else if (cnt <= stream_cap) {
            ++ctr.stream_q;
            ctr.stream_slots += cnt;
            int carry = -1;
            bool pend = false;                                            // a listed start whose count waits for the next start
            uint32_t pend_rank = 0, pend_at = 0;
            for (uint32_t r = 0; r < cnt; r += NG_LOADS * WAVE) {
                int b[NG_LOADS];
                ng_stream_trip(T, SA, n, w, r, b);
#pragma unroll
                for (int t = 0; t < NG_LOADS; ++t) {
                    const uint32_t first = r + (uint32_t)t * WAVE, i = first + l;
                    int left = __shfl_up(b[t], 1, WAVE);
                    if (l == 0) left = carry;
                    carry = __shfl(b[t], WAVE - 1, WAVE);
                    const bool start = i < cnt && b[t] != left, list = start && b[t] < TK_END;
                    const uint64_t bs = __ballot(start), bl = __ballot(list);
                    if (!bs) continue;
                    if (EMIT) {
                        if (pend && l == 0) tok_emit_count(counts, o, pend_rank, capacity, first + (uint32_t)(__ffsll((unsigned long long)bs) - 1) - pend_at);
                        const uint64_t above = l == WAVE - 1 ? 0ull : bs & ~((2ull << l) - 1ull);
                        if (list) {
                            const uint32_t rank = listed + (uint32_t)__popcll(bl & below);
                            tok_emit_token(toks, o, rank, capacity, b[t]);
                            if (above) tok_emit_count(counts, o, rank, capacity, first + (uint32_t)(__ffsll((unsigned long long)above) - 1) - i);
                        }
                        const int last = 63 - __clzll((unsigned long long)bs);
                        pend = (bl >> last) & 1ull;
                        pend_rank = listed + (uint32_t)__popcll(bl & ((1ull << last) - 1ull));
                        pend_at = first + (uint32_t)last;
                    }
                    listed += (uint32_t)__popcll(bl);
                }
            }
            if (EMIT && pend && l == 0) tok_emit_count(counts, o, pend_rank, capacity, cnt - pend_at);
        } else {
            ++ctr.search_q;
            const NgSample smp = ng_sample(T, SA, n, w);
            // the first walk counts the lane's listed starts and finds its first start (lane 0: the run that starts the range) ...
            uint32_t mine = l == 0 && smp.b < TK_END ? 1u : 0u, first_at = l == 0 ? 0u : 0xffffffffu;
            const uint32_t probes = 1 + ng_walk(T, SA, n, w, smp, [&](uint32_t u, int bv) {
                if (first_at == 0xffffffffu) first_at = u;
                mine += bv < TK_END ? 1u : 0u;
            });
            ctr.search_slots += wave_incl_sum(probes);                    // (lane 63 holds the wave's sum)
            const uint32_t incl = wave_incl_sum(mine);
            listed = (uint32_t)__shfl((int)incl, WAVE - 1, WAVE);
            if (EMIT) {                                                   // ... the second walks them again with the ranks known
                uint32_t nf = first_at;                                   // the first start of a later lane, else cnt
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) {                      // inclusive suffix minimum over the lanes
                    const uint32_t t = (uint32_t)__shfl_down((int)nf, d, WAVE);
                    if (l + d < WAVE && t < nf) nf = t;
                }
                const uint32_t nx = (uint32_t)__shfl_down((int)nf, 1, WAVE);
                const uint32_t next_first = l == WAVE - 1 || nx > cnt ? cnt : nx;
                uint32_t rank = incl - mine, pend_rank = 0, pend_at = 0;
                bool pend = false;                                        // a listed start whose count waits for the next start
                if (l == 0 && smp.b < TK_END) { tok_emit_token(toks, o, rank, capacity, smp.b); pend = true; pend_rank = rank; ++rank; }
                ng_walk(T, SA, n, w, smp, [&](uint32_t u, int bv) {
                    if (pend) tok_emit_count(counts, o, pend_rank, capacity, u - pend_at);
                    pend = bv < TK_END;
                    if (pend) { tok_emit_token(toks, o, rank, capacity, bv); pend_rank = rank; pend_at = u; ++rank; }
                });
                if (pend) tok_emit_count(counts, o, pend_rank, capacity, next_first - pend_at);
            }
        }
        if (!EMIT && l == 0) { nnz[q] = listed; at_end[q] = (uint8_t)w.ae; }
    }
    if (!EMIT) ng_flush(ctr, ctl);
}

static_assert(TK_END == sym_end<uint16_t>(), "TK_END is the token alphabet's sentinel");
static_assert((int)TK_LIMIT_U32 == sym_end<uint32_t>(), "the ids of a 32-bit token text lie below their sentinel");

}  // namespace sa
