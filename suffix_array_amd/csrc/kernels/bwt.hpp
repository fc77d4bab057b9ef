// kernels/bwt.hpp -- Burrows-Wheeler transform from a device-resident text and suffix array, and its inverse (DESIGN.md
// section 12).  Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// Forward (SA in the layout of sa_amd_saca_u8: n + 1 entries, SA[0] = n):
//   primary = the slot i with SA[i] == 0;  B[k] = T[SA[k] - 1] for k < primary,  B[k] = T[SA[k + 1] - 1] for k >= primary.
//   k_bwt_range   range pass (entry > n, SA[0] != n, the zero entries counted and located) -- before anything reads through
//                 the entries;  k_bwt_gather   one pass: SA streamed (16-byte loads), one random text byte per slot, B streamed.
//
// Inverse.  Rows 0 .. n, row 0 the empty suffix, row(b) = b for b < primary, else b + 1.
//   k_unbwt_keys + one stable 8-bit pass of the 32-bit sort (iota values): order[k] = the k-th index of B by (B[b], b)
//   k_unbwt_psi        ψ[k + 1] = row(order[k]), ψ[0] = primary; starts[c] = 1 + #{b : B[b] < c} (the first column F as
//                      257 digit starts).  T[j] = F[ψ^j(primary)], ψ^n(primary) = 0.  ψ is a permutation whatever B holds.
//   k_unbwt_splitters  the rows whose hash is 0 mod S, and `primary`, become walkers (compacted list + row -> walker index)
//   k_unbwt_walk       one lane per walker follows ψ to the next splitter: (next walker, steps).  At most `cap` steps per
//                      launch; a lane that is not there yet saves (row, steps) and goes on from there in the next launch
//   k_unbwt_rank       pointer jumping over the m sublists, cut in front of primary's walker: D[w] = rows from w's splitter to
//                      the end of the list; k_unbwt_base: base[w] = D[primary's] - D[w].  D[primary's] != n + 1: not a transform
//   k_unbwt_write      each walker walks its sublist again and writes F[row] to T_out[base + t]
// Only ψ (a permutation of 0 .. n) is ever used as an address, so an invalid (B, primary) pair reads nothing outside the
// tables; T_out is written by k_unbwt_write alone, which runs only after the ranked chain has been seen to cover n + 1 rows.
#pragma once
#include "common.hpp"

namespace sa {

constexpr int BWT_THREADS = 256;
constexpr uint32_t UNBWT_NIL = 0xffffffffu;
constexpr unsigned long long UNBWT_DONE = ~0ull;

// uint32 words of the control slab (behind the sort scratch's error words at 0 .. 3)
constexpr int BWT_W_FLAGS = 8, BWT_W_ZEROS = 9, BWT_W_PRIMARY = 10;                   // forward: range pass
constexpr int UNBWT_W_M = 8, UNBWT_W_PIDX = 9, UNBWT_W_TOTAL = 10, UNBWT_W_TAIL = 11;   // inverse
// uint64 counters of the inverse at byte 64 of the slab
constexpr int UNBWT_C_ACTIVE = 0, UNBWT_C_STEPS = 1, UNBWT_C_LONGEST = 2, UNBWT_C_WORDS = 3;

__device__ __forceinline__ unsigned long long bwt_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// ---- forward ----

// flags bit 0: an entry > n; bit 1: SA[0] != n or n in another slot.  The zero entries are counted (one atomic per wave that
// sees any) and the highest slot that holds one is kept.  Whole waves in every iteration (ballot).
__global__ __launch_bounds__(BWT_THREADS) void k_bwt_range(const uint32_t *__restrict__ SA, int64_t n, uint32_t *__restrict__ ctl)
{
    const int64_t stride = (int64_t)gridDim.x * BWT_THREADS;
    const int64_t top = (n + 1 + stride - 1) / stride * stride;
    uint32_t f = 0;
    for (int64_t i = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x; i < top; i += stride) {
        bool zero = false;
        if (i <= n) {
            const uint32_t s = SA[i];
            if ((int64_t)s > n) f |= 1u;
            if ((i == 0) != ((int64_t)s == n)) f |= 2u;
            zero = s == 0u && n > 0;
        }
        const uint64_t m = __ballot(zero);
        if (m) {
            if (lane_id() == __builtin_ctzll(m)) atomicAdd(&ctl[BWT_W_ZEROS], (uint32_t)__popcll(m));
            if (zero) atomicMax(&ctl[BWT_W_PRIMARY], (uint32_t)i);
        }
    }
    if (f) atomicOr(&ctl[BWT_W_FLAGS], f);
}

// Four consecutive slots of B per lane: SA[k0 .. k0 + 4] (one 16-byte load where the array is aligned and the words exist, the
// fifth word only where the row of the whole text lies at or in front of the lane's slots), one text byte each, one 4-byte store
// where B is aligned.  Every entry is <= n (range pass) and the only zero is at `primary`, which no slot reads; a zero met
// anyway (cannot happen) gives a 0 byte, not a load in front of the text.
__global__ __launch_bounds__(BWT_THREADS) void k_bwt_gather(const uint8_t *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n,
                                                            int64_t primary, uint8_t *__restrict__ B, int sa_vec, int b_vec)
{
    const int64_t groups = (n + 3) >> 2;
    const int64_t stride = (int64_t)gridDim.x * BWT_THREADS;
    for (int64_t g = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x; g < groups; g += stride) {
        const int64_t k0 = g << 2;
        uint32_t v[5];
        if (sa_vec && k0 + 3 <= n) {
            const uint4 a = *(const uint4 *)(SA + k0);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = k0 + j <= n ? SA[k0 + j] : 1u;
        }
        v[4] = (primary <= k0 + 3 && k0 + 4 <= n) ? SA[k0 + 4] : 1u;
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t s = k0 + j >= primary ? v[j + 1] : v[j];
            const uint32_t c = (k0 + j < n && s != 0u) ? (uint32_t)T[(int64_t)s - 1] : 0u;
            w |= c << (8 * j);
        }
        if (b_vec && k0 + 4 <= n) *(uint32_t *)(B + k0) = w;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (k0 + j < n) B[k0 + j] = (uint8_t)(w >> (8 * j));
        }
    }
}

// ---- inverse ----

// B widened into the 32-bit keys of the sort, four per lane (keys is 16-byte aligned; B may sit at any byte address: its words
// are read whole only where they are aligned and end inside B)
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_keys(const uint8_t *__restrict__ B, int64_t n, uint32_t *__restrict__ keys, int b_vec)
{
    const int64_t groups = (n + 3) >> 2;
    const int64_t stride = (int64_t)gridDim.x * BWT_THREADS;
    for (int64_t g = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x; g < groups; g += stride) {
        const int64_t k0 = g << 2;
        if (k0 + 4 <= n) {
            uint32_t w;
            if (b_vec) w = *(const uint32_t *)(B + k0);
            else w = (uint32_t)B[k0] | ((uint32_t)B[k0 + 1] << 8) | ((uint32_t)B[k0 + 2] << 16) | ((uint32_t)B[k0 + 3] << 24);
            *(uint4 *)(keys + k0) = make_uint4(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, w >> 24);
        } else {
            for (int64_t k = k0; k < n; ++k) keys[k] = B[k];
        }
    }
}

// sorted: the keys in sorted order (the first column without row 0); order: the indices of B in that order (nullptr: the
// identity -- a sort of fewer than two pairs moves nothing).  ψ[k + 1] = row(order[k]), ψ[0] = primary;
// starts[c] = 1 + #{b : B[b] < c} for c = 0 .. 256, written by the lanes that see a digit change (and the last lane)
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_psi(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ order, int64_t n,
                                                           uint32_t primary, uint32_t *__restrict__ psi, uint32_t *__restrict__ starts)
{
    const int64_t stride = (int64_t)gridDim.x * BWT_THREADS;
    for (int64_t k = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x; k < n; k += stride) {
        const uint32_t o = order ? order[k] : (uint32_t)k;
        psi[k + 1] = o < primary ? o : o + 1u;
        const int cur = (int)(sorted[k] & 255u);
        const int prev = k ? (int)(sorted[k - 1] & 255u) : -1;
        for (int c = prev + 1; c <= cur; ++c) starts[c] = (uint32_t)(k + 1);
        if (k == n - 1) for (int c = cur + 1; c <= 256; ++c) starts[c] = (uint32_t)(n + 1);
        if (k == 0) psi[0] = primary;
    }
}

// two rounds of multiply - xorshift over the row number and the attempt's seed
__device__ __forceinline__ uint32_t unbwt_hash(uint32_t row, uint32_t seed)
{
    uint32_t h = row + seed * 0x9e3779b9u;
    h ^= h >> 16; h *= 0x7feb352du;
    h ^= h >> 15; h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ bool unbwt_is_splitter(uint32_t row, uint32_t primary, uint32_t mask, uint32_t seed)
{
    return row == primary || (unbwt_hash(row, seed) & mask) == 0u;
}

// the splitters of rows 0 .. n, compacted (one atomic per wave): srow[w] = row, widx[row] = w; the walker of `primary` posts
// its index.  A list longer than mcap is counted, not written (the host refuses it).
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_splitters(int64_t rows, uint32_t primary, uint32_t mask, uint32_t seed,
                                                                 uint32_t *__restrict__ srow, uint32_t *__restrict__ widx, uint32_t mcap,
                                                                 uint32_t *__restrict__ ctl)
{
    const int64_t stride = (int64_t)gridDim.x * BWT_THREADS;
    const int64_t top = (rows + stride - 1) / stride * stride;
    for (int64_t r = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x; r < top; r += stride) {
        const bool want = r < rows && unbwt_is_splitter((uint32_t)r, primary, mask, seed);
        const uint64_t m = __ballot(want);
        if (!m) continue;
        const int leader = __builtin_ctzll(m);
        uint32_t base = 0;
        if (lane_id() == leader) base = atomicAdd(&ctl[UNBWT_W_M], (uint32_t)__popcll(m));
        base = __shfl(base, leader, WAVE);
        if (!want) continue;
        const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
        if (slot < mcap) {
            srow[slot] = (uint32_t)r;
            widx[r] = slot;
            if ((uint32_t)r == primary) ctl[UNBWT_W_PIDX] = slot;
        }
    }
}

// One lane per walker.  first: the walk starts at the walker's splitter; else it goes on from the saved (row, steps), unless the
// state says UNBWT_DONE.  Arrival at a splitter: link[w] = (walker of that splitter, or NIL when it is primary's: the list is cut
// there) | steps << 32.  The counters: lanes still walking, steps of this launch, the longest finished walk.
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_walk(const uint32_t *__restrict__ psi, uint32_t primary, uint32_t mask, uint32_t seed,
                                                            const uint32_t *__restrict__ srow, const uint32_t *__restrict__ widx,
                                                            unsigned long long *__restrict__ link, unsigned long long *__restrict__ state,
                                                            int64_t m, int64_t cap, int first, unsigned long long *__restrict__ ctl)
{
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    unsigned long long took = 0, active = 0, longest = 0;
    if (w < m) {
        unsigned long long s = first ? (unsigned long long)srow[w] : state[w];
        if (s != UNBWT_DONE) {
            uint32_t row = (uint32_t)s;
            unsigned long long steps = s >> 32;
            bool there = false;
            for (int64_t q = 0; q < cap; ++q) {
                row = psi[row];
                ++steps; ++took;
                if (unbwt_is_splitter(row, primary, mask, seed)) { there = true; break; }
            }
            if (there) {
                link[w] = (unsigned long long)(row == primary ? UNBWT_NIL : widx[row]) | (steps << 32);
                state[w] = UNBWT_DONE;
                longest = steps;
            } else {
                state[w] = (unsigned long long)row | (steps << 32);
                active = 1;
            }
        }
    }
    took = bwt_wave_sum(took);
    active = bwt_wave_sum(active);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(longest, o, WAVE); longest = longest > t ? longest : t; }
    if (lane_id() == 0) {
        if (took) atomicAdd(&ctl[UNBWT_C_STEPS], took);
        if (active) atomicAdd(&ctl[UNBWT_C_ACTIVE], active);
        if (longest) atomicMax(&ctl[UNBWT_C_LONGEST], longest);
    }
}

// one round of pointer jumping: (next, d) of w becomes (next of next, d + d of next).  After ceil(log2 m) rounds every walker
// on primary's list points at NIL and d is the number of rows from its splitter to the end of the list.  (32-bit sums: a valid
// list holds n + 1 <= 2^31 rows; on the closed cycles of an invalid input they wrap, and the result is refused anyway.)
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_rank(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out, int64_t m)
{
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    if (w >= m) return;
    unsigned long long a = in[w];
    const uint32_t nx = (uint32_t)a;
    if (nx != UNBWT_NIL) {
        const unsigned long long b = in[nx];
        a = (unsigned long long)(uint32_t)b | ((unsigned long long)((uint32_t)(a >> 32) + (uint32_t)(b >> 32)) << 32);
    }
    out[w] = a;
}

// base[w] = D[primary's walker] - D[w]: the text position of the walker's splitter row; primary's walker posts (D, next)
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_base(const unsigned long long *__restrict__ ranked, int64_t m, uint32_t pidx,
                                                            uint32_t *__restrict__ base, uint32_t *__restrict__ ctl)
{
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    if (w >= m) return;
    const unsigned long long p = ranked[pidx];
    base[w] = (uint32_t)(p >> 32) - (uint32_t)(ranked[w] >> 32);
    if (w == (int64_t)pidx) { ctl[UNBWT_W_TOTAL] = (uint32_t)(p >> 32); ctl[UNBWT_W_TAIL] = (uint32_t)p; }
}

// One lane per walker, again along its sublist: T_out[base + t] = F[row], F by binary search in the 257 digit starts (LDS).  The
// lane's row and position are kept in srow / base themselves, so a launch of at most `cap` steps goes on where the one before
// stopped; base = NIL marks a finished walker.  Row 0 (position n, the sentinel's place) writes nothing, and no position >= n.
__global__ __launch_bounds__(BWT_THREADS) void k_unbwt_write(const uint32_t *__restrict__ psi, uint32_t primary, uint32_t mask, uint32_t seed,
                                                             uint32_t *__restrict__ srow, uint32_t *__restrict__ base, int64_t m, int64_t n,
                                                             const uint32_t *__restrict__ starts, uint8_t *__restrict__ T_out, int64_t cap,
                                                             unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t s_starts[257];
    for (int i = threadIdx.x; i < 257; i += BWT_THREADS) s_starts[i] = starts[i];
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    unsigned long long took = 0;
    if (w < m) {
        uint32_t j = base[w];
        if (j != UNBWT_NIL) {
            uint32_t row = srow[w];
            bool there = false;
            for (int64_t q = 0; q < cap; ++q) {
                if (row != 0u && (int64_t)j < n) {
                    int c = 0;
#pragma unroll
                    for (int step = 128; step > 0; step >>= 1) if (s_starts[c + step] <= row) c += step;
                    T_out[j] = (uint8_t)c;
                }
                row = psi[row];
                ++j; ++took;
                if (unbwt_is_splitter(row, primary, mask, seed)) { there = true; break; }
            }
            srow[w] = row;
            base[w] = there ? UNBWT_NIL : j;
        }
    }
    took = bwt_wave_sum(took);
    if (lane_id() == 0 && took) atomicAdd(&ctl[UNBWT_C_STEPS], took);
}

}  // namespace sa
