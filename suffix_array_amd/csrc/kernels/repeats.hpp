// kernels/repeats.hpp -- repeated substrings from a device-resident text and its suffix array.
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// T has n bytes; SA and LCP are in the layout of sa_amd_saca_u8 / sa_amd_lcp (n + 1 entries each), LCP[n + 1] reads as 0.
//   LR[p]  (n entries, text order) = length of the longest substring starting at p that also starts at some q != p;
//          LR[SA[i]] = max(LCP[i], LCP[i + 1]) for 1 <= i <= n.  p + LR[p] <= n and never decreases with p.
//   spans, mode ALL (min_len = k): the union of [p, p + LR[p]) over all p with LR[p] >= k, as maximal intervals [start, end),
//          ascending, disjoint and not adjacent.
//   spans, mode KEEP_FIRST: p is flagged iff T[p .. p + k) == T[q .. q + k) for some q < p; the union of [p, p + k) over the
//          flagged p.  The maximal slot runs [a, b] with LCP[a + 1 .. b] >= k hold the suffixes that share their first k bytes:
//          every member of a run except the one with the smallest SA value is flagged.
//
// The front end is the LCP array's (kernels/lcp.hpp) up to and including k_lcp_scan, which leaves PLCP in text order.
//   k_rep_slots      one lane per slot i = 1 .. n: l = PLCP[SA[i]], the right neighbour's from the next lane (LDS at wave and tile
//                    edges), lr = max(l, l'); LR[SA[i]] = lr by plain stores, or the pair (SA[i], lr) for the binned scatter, or
//                    (KEEP_FIRST) l in slot order plus the tile's words of the segmented minimum.  Sum and maximum of LCP and
//                    the smallest position that attains the maximum: one atomic each per tile.
//   k_rep_seg_spine  the tiles' words -> what every tile takes over from the run that enters it from the left / from the right
//   k_rep_mark       segmented minimum of SA over the runs, both directions inside the tile: flag[SA[i]] = 1 where SA[i] is not
//                    its run's minimum
//   k_rep_reach_max  reach(p) = p + LR[p] (ALL, LR[p] >= k) or p + k (KEEP_FIRST, flagged), else 0: maximum per tile
//   k_rep_spans<0>   x is covered iff max(reach[0 .. x]) > x; a start is a covered x behind an uncovered one: starts per tile,
//                    covered bytes, flagged positions
//   k_rep_spans<1>   the same again with the starts in front of the tile known: span c starts at its start and ends at the first
//                    uncovered x behind it (or n)
// A wrong permutation gives unspecified answers; every index taken from SA is checked against n before it is used and every
// reach is clamped to n, so nothing is read or written outside the tables.
#pragma once
#include "lcp.hpp"

namespace sa {

constexpr int REP_THREADS = 256;
constexpr int REP_ITEMS = 8;
constexpr int REP_TILE = REP_THREADS * REP_ITEMS;        // slots (k_rep_slots, k_rep_mark) or positions (the span kernels) per tile
constexpr int REP_WAVES = REP_THREADS / WAVE;
constexpr int REP_SPINE_THREADS = 1024;
constexpr uint32_t REP_INF = 0xffffffffu;

constexpr int REP_MODE_ALL = 0, REP_MODE_KEEP_FIRST = 1;
constexpr int REP_OUT_PLAIN = 0, REP_OUT_PAIRS = 1, REP_OUT_SLOTS = 2;

// control words (uint64) in the LCP control slab, behind the LCP_C_* words
constexpr int REP_C_SUM = 0, REP_C_BEST = 1, REP_C_COVERED = 2, REP_C_FLAGGED = 3, REP_C_SPANS = 4, REP_C_WORDS = 5;

__device__ __forceinline__ uint32_t rep_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// Slot i = 1 + blockIdx.x * REP_TILE + k * REP_THREADS + threadIdx.x.  OUT = PLAIN: out0 = LR; PAIRS: out0 = keys, out1 = values
// (entry i - 1 of each); SLOTS: out0 = LCP in slot order (entry i - 1), agg = three words per tile: a head (a slot whose LCP is
// below k: it starts a run) in the tile, minimum of SA in front of the first head, minimum of SA from the last head on.
template <int OUT>
__global__ __launch_bounds__(REP_THREADS) void k_rep_slots(const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ plcp,
                                                            uint32_t *__restrict__ out0, uint32_t *__restrict__ out1, uint32_t k_min,
                                                            uint32_t *__restrict__ agg, unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t s_edge[REP_ITEMS + 1][REP_WAVES];
    __shared__ unsigned long long s_sum[REP_WAVES], s_best[REP_WAVES];
    __shared__ uint32_t s_first, s_last, s_pre, s_post;
    const int t = threadIdx.x, l = lane_id(), w = wave_id();
    const int64_t base = (int64_t)blockIdx.x * REP_TILE + 1;
    uint32_t s[REP_ITEMS], v[REP_ITEMS];
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const int64_t i = base + (int64_t)k * REP_THREADS + t;
        s[k] = i <= n ? SA[i] : REP_INF;
    }
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) v[k] = (int64_t)s[k] < n ? plcp[s[k]] : 0u;
    if (OUT == REP_OUT_SLOTS && t == 0) { s_first = REP_INF; s_last = 0; s_pre = REP_INF; s_post = REP_INF; }
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) s_edge[k][w] = v[k];
    }
    if (t == 0) {                                            // the halo: the first slot of the next tile
        const int64_t i = base + REP_TILE;
        const uint32_t h = i <= n ? SA[i] : REP_INF;
        s_edge[REP_ITEMS][0] = (int64_t)h < n ? plcp[h] : 0u;
    }
    __syncthreads();
    unsigned long long sum = 0, best = 0;
    uint32_t first = REP_INF, last = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        uint32_t r = __shfl_down(v[k], 1, WAVE);
        if (l == WAVE - 1) r = w + 1 < REP_WAVES ? s_edge[k][w + 1] : s_edge[k + 1][0];
        const uint32_t lr = v[k] > r ? v[k] : r;
        const int64_t i = base + (int64_t)k * REP_THREADS + t;
        if ((int64_t)s[k] < n) {
            sum += v[k];
            const unsigned long long key = ((unsigned long long)lr << 32) | (uint32_t)~s[k];
            best = best > key ? best : key;
            if (OUT == REP_OUT_PLAIN) out0[s[k]] = lr;
        }
        if (OUT == REP_OUT_PAIRS && i <= n) { out0[i - 1] = s[k]; out1[i - 1] = lr; }
        if (OUT == REP_OUT_SLOTS) {
            if (i <= n) out0[i - 1] = v[k];
            if (v[k] < k_min) {                              // (slots past n read as LCP 0: heads that carry no position)
                const uint32_t idx = (uint32_t)(k * REP_THREADS + t);
                first = rep_min(first, idx);
                last = last > idx ? last : idx;
            }
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, WAVE);
        const unsigned long long b2 = __shfl_xor(best, o, WAVE);
        best = best > b2 ? best : b2;
    }
    if (l == 0) { s_sum[w] = sum; s_best[w] = best; }
    if (OUT == REP_OUT_SLOTS) {
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            first = rep_min(first, __shfl_xor(first, o, WAVE));
            const uint32_t l2 = __shfl_xor(last, o, WAVE);
            last = last > l2 ? last : l2;
        }
        if (l == 0 && first != REP_INF) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long ts = 0, tb = 0;
        for (int q = 0; q < REP_WAVES; ++q) { ts += s_sum[q]; tb = tb > s_best[q] ? tb : s_best[q]; }
        if (ts) atomicAdd(&ctl[REP_C_SUM], ts);
        if (tb) atomicMax(&ctl[REP_C_BEST], tb);
    }
    if (OUT == REP_OUT_SLOTS) {
        const uint32_t f = s_first, e = s_last;              // f == REP_INF: no head in the tile, both minima are the tile's
        uint32_t pre = REP_INF, post = REP_INF;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            const uint32_t idx = (uint32_t)(k * REP_THREADS + t);
            if (idx < f) pre = rep_min(pre, s[k]);
            if (f == REP_INF || idx >= e) post = rep_min(post, s[k]);
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            pre = rep_min(pre, __shfl_xor(pre, o, WAVE));
            post = rep_min(post, __shfl_xor(post, o, WAVE));
        }
        if (l == 0) { atomicMin(&s_pre, pre); atomicMin(&s_post, post); }
        __syncthreads();
        if (t == 0) {
            agg[3 * (int64_t)blockIdx.x] = f != REP_INF ? 1u : 0u;
            agg[3 * (int64_t)blockIdx.x + 1] = s_pre;
            agg[3 * (int64_t)blockIdx.x + 2] = s_post;
        }
    }
}

// The segmented-minimum operator on (head seen, minimum since the last head): x then y.
__device__ __forceinline__ void rep_seg_join(bool &yf, uint32_t &yv, bool xf, uint32_t xv)
{
    if (!yf) yv = rep_min(yv, xv);
    yf = yf || xf;
}

// Exclusive scan of that operator over the THREADS threads of a workgroup, in thread order or (REV) against it: returns what
// reaches this thread from the threads in front of it (REP_INF: nothing).  lds_f, lds_v: THREADS / 64 words each.
template <int THREADS, bool REV>
__device__ __forceinline__ uint32_t rep_block_seg_excl(bool f, uint32_t v, uint32_t *lds_f, uint32_t *lds_v)
{
    constexpr int NW = THREADS / WAVE;
    const int l = lane_id(), w = wave_id();
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int src = REV ? l + o : l - o;
        const uint32_t v2 = __shfl(v, src & (WAVE - 1), WAVE);
        const int f2 = __shfl((int)f, src & (WAVE - 1), WAVE);
        if (REV ? src < WAVE : src >= 0) rep_seg_join(f, v, f2 != 0, v2);
    }
    if (l == (REV ? 0 : WAVE - 1)) { lds_f[w] = f ? 1u : 0u; lds_v[w] = v; }
    __syncthreads();
    uint32_t c = REP_INF;                                    // what enters this wave
    if (REV) { for (int q = NW - 1; q > w; --q) c = lds_f[q] ? lds_v[q] : rep_min(c, lds_v[q]); }
    else { for (int q = 0; q < w; ++q) c = lds_f[q] ? lds_v[q] : rep_min(c, lds_v[q]); }
    __syncthreads();
    const uint32_t inc = f ? v : rep_min(c, v);
    const int nb = REV ? l + 1 : l - 1;
    const uint32_t ex = __shfl(inc, nb & (WAVE - 1), WAVE);
    return (REV ? nb < WAVE : nb >= 0) ? ex : c;
}

// Two workgroups.  Block 0: carry[2 t] = the minimum of SA over the part of the run entering tile t from the left (the slots in
// front of the tile back to the nearest head, that head included); block 1: carry[2 t + 1] = over the part that goes on behind
// the tile (up to the next head, which is not included).  REP_INF where there is none.
__global__ __launch_bounds__(REP_SPINE_THREADS) void k_rep_seg_spine(const uint32_t *__restrict__ agg, int64_t tiles, uint32_t *__restrict__ carry)
{
    __shared__ uint32_t lds_f[REP_SPINE_THREADS / WAVE], lds_v[REP_SPINE_THREADS / WAVE];
    const bool rev = blockIdx.x == 1;
    const int t = threadIdx.x;
    const int64_t per = (tiles + REP_SPINE_THREADS - 1) / REP_SPINE_THREADS;
    int64_t b = (int64_t)t * per, e = b + per;
    if (b > tiles) b = tiles;
    if (e > tiles) e = tiles;
    // the chunk's own word: its tiles joined in the direction of travel
    bool f = false;
    uint32_t v = REP_INF;
    if (!rev) { for (int64_t i = b; i < e; ++i) { const bool hf = agg[3 * i] != 0; const uint32_t hv = agg[3 * i + 2]; v = hf ? hv : rep_min(v, hv); f = f || hf; } }
    else { for (int64_t i = e - 1; i >= b; --i) { const bool hf = agg[3 * i] != 0; const uint32_t hv = agg[3 * i + 1]; v = hf ? hv : rep_min(v, hv); f = f || hf; } }
    uint32_t run = rev ? rep_block_seg_excl<REP_SPINE_THREADS, true>(f, v, lds_f, lds_v)
                       : rep_block_seg_excl<REP_SPINE_THREADS, false>(f, v, lds_f, lds_v);
    if (!rev) {
        for (int64_t i = b; i < e; ++i) {
            carry[2 * i] = run;
            const uint32_t hv = agg[3 * i + 2];
            run = agg[3 * i] != 0 ? hv : rep_min(run, hv);
        }
    } else {
        for (int64_t i = e - 1; i >= b; --i) {
            carry[2 * i + 1] = run;
            const uint32_t hv = agg[3 * i + 1];
            run = agg[3 * i] != 0 ? hv : rep_min(run, hv);
        }
    }
}

// Slots 1 + blockIdx.x * REP_TILE + threadIdx.x * REP_ITEMS + k: the minimum of SA over the slot's whole run = min(what reaches
// it from the left, what reaches it from the right); a member that is not the minimum is a later copy: flag[SA[i]] = 1.
__global__ __launch_bounds__(REP_THREADS) void k_rep_mark(const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ lcps,
                                                           uint32_t k_min, const uint32_t *__restrict__ carry, uint8_t *__restrict__ flag)
{
    __shared__ uint32_t lds_f[REP_WAVES], lds_v[REP_WAVES];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)t * REP_ITEMS + 1;
    uint32_t s[REP_ITEMS], fw[REP_ITEMS];
    bool head[REP_ITEMS];
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const int64_t i = i0 + k;
        s[k] = i <= n ? SA[i] : REP_INF;
        head[k] = i <= n ? lcps[i - 1] < k_min : true;
        if ((int64_t)s[k] >= n) s[k] = REP_INF;
    }
    // thread words: forward = (a head, minimum from the last head on), backward = (a head, minimum in front of the first head)
    bool any = false;
    uint32_t post = REP_INF, pre = REP_INF;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        if (!any && !head[k]) pre = rep_min(pre, s[k]);
        post = head[k] ? s[k] : rep_min(post, s[k]);
        any = any || head[k];
    }
    // what enters the tile joins the first thread's word (forward) and the last thread's (backward): the scans carry it as far
    // as the heads let it go
    const uint32_t tile_f = carry[2 * (int64_t)blockIdx.x], tile_b = carry[2 * (int64_t)blockIdx.x + 1];
    if (t == 0 && !any) post = rep_min(post, tile_f);
    if (t == REP_THREADS - 1 && !any) pre = rep_min(pre, tile_b);
    const uint32_t cf = rep_block_seg_excl<REP_THREADS, false>(any, post, lds_f, lds_v);
    const uint32_t cb = rep_block_seg_excl<REP_THREADS, true>(any, pre, lds_f, lds_v);
    uint32_t run = t == 0 ? tile_f : cf;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) { run = head[k] ? s[k] : rep_min(run, s[k]); fw[k] = run; }
    run = t == REP_THREADS - 1 ? tile_b : cb;
#pragma unroll
    for (int k = REP_ITEMS - 1; k >= 0; --k) {
        run = rep_min(run, s[k]);
        const uint32_t mn = rep_min(run, fw[k]);
        if (s[k] != REP_INF && s[k] != mn) flag[s[k]] = 1;
        if (head[k]) run = REP_INF;
    }
}

// reach of position p: one past the last byte its repeat covers, at most n; 0 when p is not flagged
template <int MODE>
__device__ __forceinline__ uint32_t rep_reach(uint32_t raw, int64_t p, int64_t n, uint32_t k_min)
{
    const bool on = MODE == REP_MODE_ALL ? raw >= k_min : raw != 0;
    if (!on) return 0u;
    const int64_t r = p + (int64_t)(MODE == REP_MODE_ALL ? raw : k_min);
    return (uint32_t)(r < n ? r : n);
}

// REP_ITEMS consecutive positions from j0 on: LR (uint32, two 16-byte loads) or the flags (bytes, one 8-byte load); src is
// 16-byte aligned
template <int MODE>
__device__ __forceinline__ void rep_load(const void *src, int64_t j0, int64_t n, uint32_t k_min, uint32_t *x)
{
    static_assert(REP_ITEMS == 8, "two uint4 / one uint2 per thread");
    if (MODE == REP_MODE_ALL) {
        const uint32_t *v = (const uint32_t *)src;
        if (j0 + REP_ITEMS <= n) {
            const uint4 a = *(const uint4 *)(v + j0), b = *(const uint4 *)(v + j0 + 4);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < REP_ITEMS; ++k) x[k] = j0 + k < n ? v[j0 + k] : 0u;
        }
    } else {
        const uint8_t *v = (const uint8_t *)src;
        if (j0 + REP_ITEMS <= n) {
            const uint2 a = *(const uint2 *)(v + j0);
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[k] = (a.x >> (8 * k)) & 255u; x[4 + k] = (a.y >> (8 * k)) & 255u; }
        } else {
#pragma unroll
            for (int k = 0; k < REP_ITEMS; ++k) x[k] = j0 + k < n ? v[j0 + k] : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) x[k] = j0 + k < n ? rep_reach<MODE>(x[k], j0 + k, n, k_min) : 0u;
}

template <int MODE>
__global__ __launch_bounds__(REP_THREADS) void k_rep_reach_max(const void *__restrict__ src, int64_t n, uint32_t k_min, uint32_t *__restrict__ tile_max)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    uint32_t x[REP_ITEMS];
    rep_load<MODE>(src, (int64_t)blockIdx.x * REP_TILE + (int64_t)threadIdx.x * REP_ITEMS, n, k_min, x);
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) mx = mx > x[k] ? mx : x[k];
    uint32_t all;
    (void)block_incl_max<REP_THREADS>(mx, lds, &all);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = all;
}

// one workgroup: cnt -> exclusive running sum in place, the total to *total
__global__ __launch_bounds__(REP_SPINE_THREADS) void k_rep_sum_spine(uint32_t *__restrict__ cnt, int64_t tiles, unsigned long long *__restrict__ total)
{
    __shared__ uint32_t lds[REP_SPINE_THREADS / WAVE + 1];
    const int t = threadIdx.x;
    const int64_t per = (tiles + REP_SPINE_THREADS - 1) / REP_SPINE_THREADS;
    int64_t b = (int64_t)t * per, e = b + per;
    if (b > tiles) b = tiles;
    if (e > tiles) e = tiles;
    uint32_t sum = 0;
    for (int64_t i = b; i < e; ++i) sum += cnt[i];
    uint32_t all;
    uint32_t run = block_excl_sum<REP_SPINE_THREADS>(sum, lds, &all);
    for (int64_t i = b; i < e; ++i) { const uint32_t c = cnt[i]; cnt[i] = run; run += c; }
    if (t == 0) *total = all;
}

// WRITE = 0: cnt[tile] = starts in the tile; covered bytes and flagged positions to ctl.  WRITE = 1: cnt holds the starts in
// front of every tile; the first `capacity` spans to spans[2 c] (start), spans[2 c + 1] (end).  carry: exclusive running
// maximum of the tiles' reach (k_lcp_scan_spine over k_rep_reach_max's words).
template <int MODE, int WRITE>
__global__ __launch_bounds__(REP_THREADS) void k_rep_spans(const void *__restrict__ src, int64_t n, uint32_t k_min, const uint32_t *__restrict__ carry,
                                                            uint32_t *__restrict__ cnt, uint32_t *__restrict__ spans, int64_t capacity,
                                                            unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    __shared__ uint32_t s_inc[REP_THREADS];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)t * REP_ITEMS;
    uint32_t x[REP_ITEMS];
    rep_load<MODE>(src, j0, n, k_min, x);
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) mx = mx > x[k] ? mx : x[k];
    uint32_t all;
    s_inc[t] = block_incl_max<REP_THREADS>(mx, lds, &all);
    __syncthreads();
    uint32_t run = carry[blockIdx.x];
    if (t) run = run > s_inc[t - 1] ? run : s_inc[t - 1];
    // bit k of st / en: position j0 + k starts a span / is the first uncovered position behind one
    uint32_t st = 0, en = 0, cov = 0, flg = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const int64_t p = j0 + k;
        const bool prev = p > 0 && (int64_t)run >= p;         // max(reach[0 .. p - 1]) > p - 1
        run = run > x[k] ? run : x[k];
        const bool now = p < n && (int64_t)run > p;
        if (now && !prev) st |= 1u << k;
        if (prev && !now && p < n) en |= 1u << k;
        cov += now ? 1u : 0u;
        flg += x[k] != 0 ? 1u : 0u;
    }
    const bool closes = j0 <= n - 1 && n - 1 < j0 + REP_ITEMS && (int64_t)run > n - 1;      // the last position is covered: its span ends at n
    uint32_t total;
    const uint32_t ex = block_excl_sum<REP_THREADS>((uint32_t)__popc(st), lds, &total);
    if (WRITE == 0) {
        if (t == 0) cnt[blockIdx.x] = total;
        lcp_block_add(cov, &ctl[REP_C_COVERED]);
        lcp_block_add(flg, &ctl[REP_C_FLAGGED]);
    } else {
        int64_t c = (int64_t)cnt[blockIdx.x] + ex;          // spans that start in front of position j0
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            if ((en >> k) & 1u) { if (c >= 1 && c - 1 < capacity) spans[2 * (c - 1) + 1] = (uint32_t)(j0 + k); }
            if ((st >> k) & 1u) { if (c < capacity) spans[2 * c] = (uint32_t)(j0 + k); ++c; }
        }
        if (closes && c >= 1 && c - 1 < capacity) spans[2 * (c - 1) + 1] = (uint32_t)n;
    }
}

}  // namespace sa
