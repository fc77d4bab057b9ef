// kernels/lz.hpp -- Lempel-Ziv factorisation from a device-resident text and its suffix array.
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// T has n bytes; SA is in the layout of sa_amd_saca_u8 (n + 1 entries, SA[0] = n).  A = SA[1 .. n] ("slots", 0-based here).
//   P(p) = A[psv(i)], N(p) = A[nsv(i)] for A[i] = p: the nearest slot to the left / right that holds a smaller value (n: none)
//   lp(p) = lcp(T[p..], T[P(p)..]), ln likewise; LPF[p] = max(lp, ln); SRC[p] = P(p) if lp >= ln, else N(p); LZ_LITERAL if LPF = 0
//   phrase starts: s_0 = 0, s_{k+1} = s_k + max(1, LPF[s_k]); phrase k = (SRC[s_k], max(1, LPF[s_k]))
//
// Stage 1, nearest smaller values.  Minima over blocks of f = 32 children, level k = minima over 32^k slots; 32 words are the
// 128 bytes of one memory request, so one step of a query reads one request's worth of siblings, and a tile of 32^2 = 1024
// slots (4 KiB of LDS plus its 32 group minima) leaves the CU's LDS to a dozen workgroups.
//   k_lz_tile   the tile in LDS: group minima (level 1) and the tile minimum (level 2) to global memory; every slot scans its
//               siblings in its group of 32, then the groups of its tile, then the group that holds the answer: at most
//               31 + 31 + 32 LDS reads a side.  The answer, or LZ_UNRES, goes out in slot order (coalesced).
//   k_lz_level  level k from level k - 1, k = 3 .. K, K the first level with at most 32 entries
//   k_lz_far    an unresolved side climbs: at level 2 .. K the siblings on its side of its block (at most 31 loads a level),
//               until one has a smaller minimum; then it descends, one block of at most 32 children a level, down to level 0.
//               AT MOST 31 (K - 1) + 32 K LOADS A QUERY, K <= 6 for n < 2^31 (347 loads), WHATEVER THE PERMUTATION: no tile is
//               scanned, and a lane's work does not depend on how many other slots resolve in the same far tile (they read the
//               same few words, which the cache serves).  Then Pphi[A[i]] = A[psv], Nphi[A[i]] = A[nsv] by plain stores.
// The minima are those of the array as it stands, so a block whose minimum is smaller always has a child whose minimum is
// smaller: with a wrong permutation (duplicates) the answers are unspecified but every index stays inside the tables.
//
// Values: the value stage of kernels/lcp.hpp runs twice, on Pphi and on Nphi (host/lz.hpp); k_lz_merge writes LPF and SRC.
//
// Phrase starts: next(p) = min(n, p + max(1, LPF[p])) points forward, the starts are the path from 0.  As the inverse
// transform of kernels/bwt.hpp walks psi: positions whose hash is 0 mod S, and position 0, are splitters (k_unbwt_splitters,
// primary = 0); k_lz_walk: one lane per splitter follows next to the following splitter or to n, at most `cap` steps a launch
// with its place saved; k_lz_jump: ceil(log2 m) rounds -- every walker known to be on the path marks the one it points at,
// then every pointer doubles (after r rounds the walkers at distance < 2^r from position 0's are marked); k_lz_flag: the marked
// walkers walk again and flag their positions; k_lz_emit<0/1>: flags per tile, running sum (k_rep_sum_spine), the first
// `capacity` phrases in order.  Work: two walks of n / S expected sublists of S expected steps; dependent launches:
// (restarts + 1) * ceil(longest / cap) + log2 m, none of which depends on the text beyond the hash.
#pragma once
#include "bwt.hpp"
#include "repeats.hpp"

namespace sa {

constexpr int LZ_FAN = 32, LZ_FAN_LOG = 5;
constexpr int LZ_THREADS = 256;
constexpr int LZ_ITEMS = 4;
constexpr int LZ_TILE = LZ_THREADS * LZ_ITEMS;           // slots per tile of stage 1
constexpr int LZ_GROUPS = LZ_TILE / LZ_FAN;
constexpr int LZ_MAX_LEVELS = 8;
constexpr uint32_t LZ_NONE = 0xffffffffu;                // no smaller value on that side; also SA_AMD_LZ_LITERAL
constexpr uint32_t LZ_UNRES = 0xfffffffeu;               // not inside the tile
static_assert(LZ_TILE == LZ_FAN * LZ_FAN, "a tile is level 2");
static_assert(LZ_THREADS == LCP_THREADS, "lcp_block_add");

// control words (uint64) at byte 128 of the LCP control slab
constexpr int LZ_C_UNRES = 0, LZ_C_HSTEPS = 1, LZ_C_HMAX = 2, LZ_C_PHRASES = 3, LZ_C_LITERALS = 4, LZ_C_BEST = 5, LZ_C_WORDS = 6;

// levels 1 .. top of the minima: level k has cnt[k] words at base + off[k]
struct LzLevels {
    uint32_t *base;
    int64_t off[LZ_MAX_LEVELS], cnt[LZ_MAX_LEVELS];
    int top;
};

// LEQ_LEFT (kernels/substrings.hpp, values below 2^31): the left side asks for the nearest value <= v, as "< v + 1"; the right
// side and the minima are the same.  false: both sides ask for "< v", the arithmetic of the factorisation.
template <bool LEQ_LEFT>
__global__ __launch_bounds__(LZ_THREADS) void k_lz_tile(const uint32_t *__restrict__ A, int64_t n, uint32_t *__restrict__ psl,
                                                         uint32_t *__restrict__ nsl, uint32_t *__restrict__ lvl1, uint32_t *__restrict__ lvl2,
                                                         unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t s_a[LZ_TILE];
    __shared__ uint32_t s_m[LZ_GROUPS];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * LZ_TILE;
    uint32_t x[LZ_ITEMS];
#pragma unroll
    for (int k = 0; k < LZ_ITEMS; ++k) {
        const int idx = k * LZ_THREADS + t;
        x[k] = base + idx < n ? A[base + idx] : LZ_NONE;      // (padding is never smaller than anything)
        s_a[idx] = x[k];
        uint32_t m = x[k];
#pragma unroll
        for (int o = LZ_FAN / 2; o > 0; o >>= 1) m = rep_min(m, __shfl_xor(m, o, WAVE));
        if ((t & (LZ_FAN - 1)) == 0) s_m[idx >> LZ_FAN_LOG] = m;
    }
    __syncthreads();
    if (t < LZ_GROUPS) {
        const uint32_t m = s_m[t];
        const int64_t g = (base >> LZ_FAN_LOG) + t;
        if (g * LZ_FAN < n) lvl1[g] = m;
        uint32_t all = m;
#pragma unroll
        for (int o = LZ_GROUPS / 2; o > 0; o >>= 1) all = rep_min(all, __shfl_xor(all, o, WAVE));
        if (t == 0) lvl2[blockIdx.x] = all;
    }
    unsigned long long unres = 0;
#pragma unroll
    for (int k = 0; k < LZ_ITEMS; ++k) {
        const int idx = k * LZ_THREADS + t;
        if (base + idx >= n) continue;
        const uint32_t v = x[k];
        const uint32_t vl = LEQ_LEFT ? v + 1u : v;
        const int g = idx >> LZ_FAN_LOG, g0 = g << LZ_FAN_LOG;
        // ---- left ----
        int found = -1;
        for (int j = idx - 1; j >= g0; --j) if (s_a[j] < vl) { found = j; break; }
        if (found < 0) {
            int h = g - 1;
            while (h >= 0 && !(s_m[h] < vl)) --h;
            if (h >= 0) { found = (h << LZ_FAN_LOG) + LZ_FAN - 1; while (!(s_a[found] < vl)) --found; }
        }
        const uint32_t pl = found >= 0 ? (uint32_t)(base + found) : LZ_UNRES;
        // ---- right ----
        found = -1;
        for (int j = idx + 1; j < g0 + LZ_FAN; ++j) if (s_a[j] < v) { found = j; break; }
        if (found < 0) {
            int h = g + 1;
            while (h < LZ_GROUPS && !(s_m[h] < v)) ++h;
            if (h < LZ_GROUPS) { found = h << LZ_FAN_LOG; while (!(s_a[found] < v)) ++found; }
        }
        const uint32_t nr = found >= 0 ? (uint32_t)(base + found) : LZ_UNRES;
        psl[base + idx] = pl;
        nsl[base + idx] = nr;
        unres += (pl == LZ_UNRES || nr == LZ_UNRES) ? 1u : 0u;
    }
    lcp_block_add(unres, &ctl[LZ_C_UNRES]);
}

// out[j] = min in[32 j .. 32 j + 31]
__global__ __launch_bounds__(LZ_THREADS) void k_lz_level(const uint32_t *__restrict__ in, int64_t cnt_in, uint32_t *__restrict__ out, int64_t cnt_out)
{
    const int64_t j = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x;
    if (j >= cnt_out) return;
    uint32_t m = LZ_NONE;
    for (int c = 0; c < LZ_FAN; ++c) { const int64_t i = j * LZ_FAN + c; if (i < cnt_in) m = rep_min(m, in[i]); }
    out[j] = m;
}

// One side of one slot through the levels.  DIR = -1: left, +1: right.  Returns the slot or LZ_NONE; steps: words loaded.
template <int DIR>
__device__ __forceinline__ uint32_t lz_far_query(const uint32_t *__restrict__ A, int64_t n, const LzLevels &lv, int64_t slot, uint32_t v,
                                                 uint32_t &steps)
{
    int level = 2;
    int64_t node = slot >> (2 * LZ_FAN_LOG);
    int64_t hit = -1;
    for (;;) {
        const uint32_t *w = lv.base + lv.off[level];
        const int64_t first = node & ~(int64_t)(LZ_FAN - 1);
        int64_t last = first + LZ_FAN - 1;
        if (last >= lv.cnt[level]) last = lv.cnt[level] - 1;
        if (DIR < 0) { for (int64_t j = node - 1; j >= first; --j) { ++steps; if (w[j] < v) { hit = j; break; } } }
        else { for (int64_t j = node + 1; j <= last; ++j) { ++steps; if (w[j] < v) { hit = j; break; } } }
        if (hit >= 0 || level == lv.top) break;
        node >>= LZ_FAN_LOG;
        ++level;
    }
    if (hit < 0) return LZ_NONE;
    while (level > 0) {                                       // the nearest child of `hit` whose minimum is smaller
        --level;
        const uint32_t *w = level ? lv.base + lv.off[level] : A;
        const int64_t cnt = level ? lv.cnt[level] : n;
        const int64_t first = hit << LZ_FAN_LOG;
        int64_t last = first + LZ_FAN - 1;
        if (last >= cnt) last = cnt - 1;
        int64_t c = DIR < 0 ? last : first;
        if (DIR < 0) { for (; c > first; --c) { ++steps; if (w[c] < v) break; } }
        else { for (; c < last; ++c) { ++steps; if (w[c] < v) break; } }
        hit = c;                                              // (the last candidate is taken unread: it is the one, or the array has duplicates)
    }
    return (uint32_t)hit;
}

// SCATTER: Pphi[A[i]] = A[psv(i)], Nphi[A[i]] = A[nsv(i)] (n: none); else the finished slot arrays stay in psl / nsl.
// LEQ_LEFT: as in k_lz_tile.
template <bool SCATTER, bool LEQ_LEFT = false>
__global__ __launch_bounds__(LZ_THREADS) void k_lz_far(const uint32_t *__restrict__ A, int64_t n, uint32_t *__restrict__ psl, uint32_t *__restrict__ nsl,
                                                        LzLevels lv, uint32_t *__restrict__ Pphi, uint32_t *__restrict__ Nphi,
                                                        unsigned long long *__restrict__ ctl)
{
    const int64_t i = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x;
    unsigned long long total = 0;
    uint32_t worst = 0;
    if (i < n) {
        const uint32_t v = A[i];
        uint32_t pl = psl[i], nr = nsl[i];
        if (pl == LZ_UNRES) { uint32_t s = 0; pl = lz_far_query<-1>(A, n, lv, i, LEQ_LEFT ? v + 1u : v, s); total += s; worst = s; }
        if (nr == LZ_UNRES) { uint32_t s = 0; nr = lz_far_query<1>(A, n, lv, i, v, s); total += s; worst = worst > s ? worst : s; }
        if (SCATTER) {
            if ((int64_t)v < n) {
                Pphi[v] = pl == LZ_NONE ? (uint32_t)n : A[pl];
                Nphi[v] = nr == LZ_NONE ? (uint32_t)n : A[nr];
            }
        } else {
            psl[i] = pl;
            nsl[i] = nr;
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) { const uint32_t w2 = __shfl_xor(worst, o, WAVE); worst = worst > w2 ? worst : w2; }
    if (lane_id() == 0 && worst) atomicMax(&ctl[LZ_C_HMAX], (unsigned long long)worst);
    lcp_block_add(total, &ctl[LZ_C_HSTEPS]);
}

// LPF = max(lp, ln); SRC = P where lp >= ln, N where ln > lp, LZ_NONE (the literal mark) where both are 0.  Either output may be null.
__global__ __launch_bounds__(LZ_THREADS) void k_lz_merge(const uint32_t *__restrict__ lp, const uint32_t *__restrict__ ln, const uint32_t *__restrict__ P,
                                                          const uint32_t *__restrict__ N, int64_t n, uint32_t *__restrict__ LPF, uint32_t *__restrict__ SRC)
{
    const int64_t stride = (int64_t)gridDim.x * LZ_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; p < n; p += stride) {
        const uint32_t a = lp[p], b = ln[p];
        if (LPF) LPF[p] = a >= b ? a : b;
        if (SRC) SRC[p] = (a | b) == 0u ? LZ_NONE : (a >= b ? P[p] : N[p]);
    }
}

__device__ __forceinline__ int64_t lz_next(const uint32_t *__restrict__ lpf, int64_t n, int64_t p)
{
    const uint32_t l = lpf[p];
    const int64_t q = p + (l ? (int64_t)l : 1);
    return q < n ? q : n;
}

// One lane per walker, as k_unbwt_walk: jump[w] = the walker of the splitter the walk arrives at, UNBWT_NIL when it reaches n.
__global__ __launch_bounds__(BWT_THREADS) void k_lz_walk(const uint32_t *__restrict__ lpf, int64_t n, uint32_t mask, uint32_t seed,
                                                         const uint32_t *__restrict__ srow, const uint32_t *__restrict__ widx, uint32_t *__restrict__ jump,
                                                         unsigned long long *__restrict__ state, int64_t m, int64_t cap, int first,
                                                         unsigned long long *__restrict__ ctl)
{
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    unsigned long long took = 0, active = 0, longest = 0;
    if (w < m) {
        unsigned long long s = first ? (unsigned long long)srow[w] : state[w];
        if (s != UNBWT_DONE) {
            int64_t pos = (uint32_t)s;
            unsigned long long steps = s >> 32;
            uint32_t to = 0;
            bool there = false;
            for (int64_t q = 0; q < cap; ++q) {
                pos = lz_next(lpf, n, pos);
                ++steps; ++took;
                if (pos >= n) { to = UNBWT_NIL; there = true; break; }
                if (unbwt_is_splitter((uint32_t)pos, 0u, mask, seed)) { to = widx[pos]; there = true; break; }
            }
            if (there) { jump[w] = to; state[w] = UNBWT_DONE; longest = steps; }
            else { state[w] = (unsigned long long)pos | (steps << 32); active = 1; }
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

// One round: a walker on the path from position 0 (its own walker `pidx`, or marked) marks the walker it points at; every
// pointer doubles.  A mark set by this launch may already be seen by it: that walker is on the path too.
__global__ __launch_bounds__(BWT_THREADS) void k_lz_jump(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t *__restrict__ mark,
                                                         int64_t m, uint32_t pidx)
{
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    if (w >= m) return;
    const uint32_t a = in[w];
    if (a == UNBWT_NIL || (int64_t)a >= m) { out[w] = UNBWT_NIL; return; }
    if (w == (int64_t)pidx || mark[w]) mark[a] = 1u;
    out[w] = in[a];
}

// The walkers on the path walk again: flag[p] = 1 for every position from the walker's splitter up to the next splitter (or n).
// The place is kept in srow, UNBWT_NIL when done, so a launch of at most `cap` steps goes on where the one before stopped.
__global__ __launch_bounds__(BWT_THREADS) void k_lz_flag(const uint32_t *__restrict__ lpf, int64_t n, uint32_t mask, uint32_t seed,
                                                         uint32_t *__restrict__ srow, const uint32_t *__restrict__ mark, uint32_t pidx, int64_t m,
                                                         int64_t cap, uint8_t *__restrict__ flag, unsigned long long *__restrict__ ctl)
{
    const int64_t w = (int64_t)blockIdx.x * BWT_THREADS + threadIdx.x;
    unsigned long long took = 0;
    if (w < m && (w == (int64_t)pidx || mark[w])) {
        int64_t pos = srow[w];
        if ((uint32_t)pos != UNBWT_NIL && pos < n) {
            bool there = false;
            for (int64_t q = 0; q < cap; ++q) {
                flag[pos] = 1;
                pos = lz_next(lpf, n, pos);
                ++took;
                if (pos >= n || unbwt_is_splitter((uint32_t)pos, 0u, mask, seed)) { there = true; break; }
            }
            srow[w] = there ? UNBWT_NIL : (uint32_t)pos;
        }
    }
    took = bwt_wave_sum(took);
    if (lane_id() == 0 && took) atomicAdd(&ctl[UNBWT_C_STEPS], took);
}

// WRITE = 0: cnt[tile] = phrase starts in the tile; literals and the longest phrase (length << 32 | ~position: the first one wins)
// to ctl.  WRITE = 1: cnt holds the starts in front of every tile (k_rep_sum_spine); phrase c, c < capacity, to
// phrases[2 c] = SRC, phrases[2 c + 1] = max(1, LPF).  flag is 8-byte aligned.
template <int WRITE>
__global__ __launch_bounds__(REP_THREADS) void k_lz_emit(const uint8_t *__restrict__ flag, const uint32_t *__restrict__ lpf, const uint32_t *__restrict__ src,
                                                          int64_t n, uint32_t *__restrict__ cnt, uint32_t *__restrict__ phrases, int64_t capacity,
                                                          unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)t * REP_ITEMS;
    uint32_t bits = 0;
    if (j0 + REP_ITEMS <= n) {
        const uint2 a = *(const uint2 *)(flag + j0);
#pragma unroll
        for (int k = 0; k < 4; ++k) { bits |= ((a.x >> (8 * k)) & 1u) << k; bits |= ((a.y >> (8 * k)) & 1u) << (4 + k); }
    } else {
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) if (j0 + k < n) bits |= (uint32_t)(flag[j0 + k] & 1u) << k;
    }
    uint32_t total;
    const uint32_t ex = block_excl_sum<REP_THREADS>((uint32_t)__popc(bits), lds, &total);
    if (WRITE == 0) {
        if (t == 0) cnt[blockIdx.x] = total;
        unsigned long long lit = 0, best = 0;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            if (!((bits >> k) & 1u)) continue;
            const uint32_t l = lpf[j0 + k];
            lit += l ? 0u : 1u;
            const unsigned long long key = ((unsigned long long)(l ? l : 1u) << 32) | (uint32_t)~(uint32_t)(j0 + k);
            best = best > key ? best : key;
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) { const unsigned long long b2 = __shfl_xor(best, o, WAVE); best = best > b2 ? best : b2; }
        if (lane_id() == 0 && best) atomicMax(&ctl[LZ_C_BEST], best);
        lcp_block_add(lit, &ctl[LZ_C_LITERALS]);
    } else {
        int64_t c = (int64_t)cnt[blockIdx.x] + ex;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            if (!((bits >> k) & 1u)) continue;
            if (c < capacity) {
                const uint32_t l = lpf[j0 + k];
                phrases[2 * c] = src[j0 + k];
                phrases[2 * c + 1] = l ? l : 1u;
            }
            ++c;
        }
    }
}

}  // namespace sa
