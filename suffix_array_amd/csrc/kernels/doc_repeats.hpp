// kernels/doc_repeats.hpp -- document-aware duplicate spans over the device index.
// Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// T has n bytes, SA is in the layout of sa_amd_saca_u8, the collection is off[0 .. ndocs] (M = ndocs + 1 entries) as
// sa_amd_index_set_documents took it, min_len = k >= 1.  ds(p) = off[doc(p)], de(p) = off[doc(p) + 1].
//   member    p is a member iff its window T[p .. p + k) lies inside its document: p + k <= de(p)
//   run       a maximal slot run [a, b] with LCP[a + 1 .. b] >= k, as for KEEP_FIRST in kernels/repeats.hpp.  Non-members are
//             transparent: they break no run (the LCP of their two neighbours is still >= k) and contribute nothing.
//   rule      mn / mx = the smallest / largest member position of the run; a member p is flagged iff
//                          ANY                     OTHER
//             KEEP_FIRST   mn < p                  mn < ds(p)
//             ALL          mn < p or mx > p        mn < ds(p) or mx >= de(p)
//   spans     the union of [p, p + k) over the flagged p: the flag bytes go to the span passes of kernels/repeats.hpp as they are
//
//   k_docrep_slots      one lane per slot i = 1 .. n (the lane order of k_rep_slots): LCP in slot order, one lookup of doc(SA[i])
//                       (k_doc_of's two-level search: a sampled top level of the offsets in LDS, staged once by a workgroup
//                       that then walks over its tiles), (ds, de) in slot order -- (0, 0) for a non-member --, the tile's
//                       five words of the two segmented minima (of p and of ~p: the maximum rides the same operator), the
//                       members, sum and maximum of LCP
//   k_docrep_seg_spine  the tiles' words -> what enters every tile from the left / right, for both minima (four workgroups)
//   k_docrep_mark       both segmented minima over the runs, both directions inside the tile; the rule; flag[p] = 1 (byte stores)
//   k_docrep_account    coverage per position as k_rep_spans computes it; doc_bytes[d] += covered bytes, one atomic per
//                       workgroup, wave, thread or run of positions, whichever is the widest that lies inside one document
//   k_docrep_touched    the number of non-zero doc_bytes words
// Every position is below n < 2^31 and every sum with k is taken in 64 bits; every index taken from SA is checked against n
// before it is used and both lookups stay inside the table whatever it holds, so nothing is read or written outside the tables.
#pragma once
#include "repeats.hpp"
#include "docs.hpp"

namespace sa {

constexpr int DOCREP_ANY = 0, DOCREP_OTHER = 1;
constexpr int DOCREP_AGG = 5;              // words per tile: head present, pre / post of the minimum, pre / post of the complemented maximum
constexpr int DOCREP_CARRY = 4;            // words per tile: minimum from the left / right, complemented maximum from the left / right

// control words (uint64) in the LCP control slab, behind the REP_C_* words
constexpr int DOCREP_C_MEMBERS = 0, DOCREP_C_TOUCHED = 1, DOCREP_C_WORDS = 2;

// the value a member position enters the maximum's channel with.  REP_INF (no member) stays REP_INF; position 0 maps to REP_INF
// as well, which reads back as "largest member 0": the value that flags nobody, as position 0 itself would.
__device__ __forceinline__ uint32_t docrep_compl(uint32_t v) { return v == REP_INF ? REP_INF : ~v; }

// doc(p) for p < n as k_doc_of finds it: the sample interval in LDS (smp[k] = off[k * stride], ns entries), then between two
// samples in the global table (at most ceil(log2 stride) loads).  The same answer as doc_lookup.
__device__ __forceinline__ uint32_t docrep_lookup(const uint32_t *smp, uint32_t ns, uint32_t stride, const uint32_t *__restrict__ off, uint32_t M,
                                                  uint32_t p)
{
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

// A workgroup stages the samples (as k_doc_of does: DOC_SAMPLES entries at most) once and takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  In tile `tile` slot
// i = 1 + tile * REP_TILE + k * REP_THREADS + threadIdx.x.  lcps, dsv, dev: entry i - 1 of each; agg: DOCREP_AGG words per tile.
// A head is a slot whose LCP is below k_min (it starts a run); slots past n are heads that carry no position.
__global__ __launch_bounds__(REP_THREADS) void k_docrep_slots(const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ plcp,
                                                               const uint32_t *__restrict__ off, uint32_t M, uint32_t stride, uint32_t ns,
                                                               uint32_t k_min, uint32_t *__restrict__ lcps, uint32_t *__restrict__ dsv, uint32_t *__restrict__ dev,
                                                               uint32_t *__restrict__ agg, unsigned long long *__restrict__ ctl,
                                                               unsigned long long *__restrict__ dctl)
{
    __shared__ uint32_t s_edge[REP_ITEMS + 1][REP_WAVES];
    __shared__ unsigned long long s_sum[REP_WAVES], s_best[REP_WAVES];
    __shared__ uint32_t s_mem[REP_WAVES];
    __shared__ uint32_t s_first, s_last, s_w[4];
    __shared__ uint32_t smp[DOC_SAMPLES];                    // 32 KiB: four workgroups a CU, as many as the pass's registers allow anyway
    const int t = threadIdx.x, l = lane_id(), w = wave_id();
    for (uint32_t k = t; k < ns; k += REP_THREADS) {
        const uint64_t j = (uint64_t)k * stride;
        smp[k] = j < M ? off[j] : (uint32_t)n;
    }
    __syncthreads();
    const int64_t tiles = (n + REP_TILE - 1) / REP_TILE;
    // (what a tile leaves in LDS is read before its last barrier and written again behind the next tile's first: no barrier between tiles)
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * REP_TILE + 1;
        uint32_t s[REP_ITEMS], v[REP_ITEMS], m[REP_ITEMS];       // SA, LCP, the member's position (REP_INF: not a member)
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            const int64_t i = base + (int64_t)k * REP_THREADS + t;
            s[k] = i <= n ? SA[i] : REP_INF;
        }
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) v[k] = (int64_t)s[k] < n ? plcp[s[k]] : 0u;
        uint32_t mem = 0;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            const int64_t i = base + (int64_t)k * REP_THREADS + t;
            uint32_t ds = 0, de = 0;
            m[k] = REP_INF;
            if ((int64_t)s[k] < n) {
                const uint32_t d = docrep_lookup(smp, ns, stride, off, M, s[k]);
                if (d < M - 1) {                                 // (always, for a sound table)
                    const uint32_t e = off[d + 1];
                    if ((int64_t)s[k] + (int64_t)k_min <= (int64_t)e) { ds = off[d]; de = e; m[k] = s[k]; ++mem; }
                }
            }
            if (i <= n) { lcps[i - 1] = v[k]; dsv[i - 1] = ds; dev[i - 1] = de; }
        }
        if (t == 0) { s_first = REP_INF; s_last = 0; s_w[0] = REP_INF; s_w[1] = REP_INF; s_w[2] = REP_INF; s_w[3] = REP_INF; }
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
            if ((int64_t)s[k] < n) {
                sum += v[k];
                const unsigned long long key = ((unsigned long long)lr << 32) | (uint32_t)~s[k];
                best = best > key ? best : key;
            }
            if (v[k] < k_min) {
                const uint32_t idx = (uint32_t)(k * REP_THREADS + t);
                first = rep_min(first, idx);
                last = last > idx ? last : idx;
            }
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, WAVE);
            const unsigned long long b2 = __shfl_xor(best, o, WAVE);
            best = best > b2 ? best : b2;
            mem += __shfl_xor(mem, o, WAVE);
            first = rep_min(first, __shfl_xor(first, o, WAVE));
            const uint32_t l2 = __shfl_xor(last, o, WAVE);
            last = last > l2 ? last : l2;
        }
        if (l == 0) {
            s_sum[w] = sum; s_best[w] = best; s_mem[w] = mem;
            if (first != REP_INF) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
        }
        __syncthreads();
        if (t == 0) {
            unsigned long long ts = 0, tb = 0, tm = 0;
            for (int q = 0; q < REP_WAVES; ++q) { ts += s_sum[q]; tb = tb > s_best[q] ? tb : s_best[q]; tm += s_mem[q]; }
            if (ts) atomicAdd(&ctl[REP_C_SUM], ts);
            if (tb) atomicMax(&ctl[REP_C_BEST], tb);
            if (tm) atomicAdd(&dctl[DOCREP_C_MEMBERS], tm);
        }
        const uint32_t f = s_first, e = s_last;                  // f == REP_INF: no head in the tile, pre and post are both the tile's
        uint32_t pre = REP_INF, post = REP_INF, prex = REP_INF, postx = REP_INF;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            const uint32_t idx = (uint32_t)(k * REP_THREADS + t);
            const uint32_t c = docrep_compl(m[k]);
            if (idx < f) { pre = rep_min(pre, m[k]); prex = rep_min(prex, c); }
            if (f == REP_INF || idx >= e) { post = rep_min(post, m[k]); postx = rep_min(postx, c); }
        }
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            pre = rep_min(pre, __shfl_xor(pre, o, WAVE));
            post = rep_min(post, __shfl_xor(post, o, WAVE));
            prex = rep_min(prex, __shfl_xor(prex, o, WAVE));
            postx = rep_min(postx, __shfl_xor(postx, o, WAVE));
        }
        if (l == 0) { atomicMin(&s_w[0], pre); atomicMin(&s_w[1], post); atomicMin(&s_w[2], prex); atomicMin(&s_w[3], postx); }
        __syncthreads();
        if (t == 0) {
            uint32_t *a = agg + DOCREP_AGG * tile;
            a[0] = f != REP_INF ? 1u : 0u;
            a[1] = s_w[0]; a[2] = s_w[1]; a[3] = s_w[2]; a[4] = s_w[3];
        }
    }
}

// Four workgroups, blockIdx.x = 2 * channel + direction (channel 0: the minimum, 1: the complemented maximum).  Direction 0:
// carry[4 t + 2 c] = the channel's minimum over the part of the run that enters tile t from the left (back to the nearest head,
// that head included); direction 1: carry[4 t + 2 c + 1] = over the part that goes on behind the tile (up to the next head,
// which is not included).  REP_INF where there is none.  The two directions of k_rep_seg_spine, once per channel.
__global__ __launch_bounds__(REP_SPINE_THREADS) void k_docrep_seg_spine(const uint32_t *__restrict__ agg, int64_t tiles, uint32_t *__restrict__ carry)
{
    __shared__ uint32_t lds_f[REP_SPINE_THREADS / WAVE], lds_v[REP_SPINE_THREADS / WAVE];
    const bool rev = (blockIdx.x & 1u) != 0;
    const int ch = (int)(blockIdx.x >> 1);
    const int src = 1 + 2 * ch + (rev ? 0 : 1);              // forward: the tile's post word; backward: its pre word
    const int dst = 2 * ch + (rev ? 1 : 0);
    const int t = threadIdx.x;
    const int64_t per = (tiles + REP_SPINE_THREADS - 1) / REP_SPINE_THREADS;
    int64_t b = (int64_t)t * per, e = b + per;
    if (b > tiles) b = tiles;
    if (e > tiles) e = tiles;
    bool f = false;
    uint32_t v = REP_INF;
    if (!rev) { for (int64_t i = b; i < e; ++i) { const bool hf = agg[DOCREP_AGG * i] != 0; const uint32_t hv = agg[DOCREP_AGG * i + src]; v = hf ? hv : rep_min(v, hv); f = f || hf; } }
    else { for (int64_t i = e - 1; i >= b; --i) { const bool hf = agg[DOCREP_AGG * i] != 0; const uint32_t hv = agg[DOCREP_AGG * i + src]; v = hf ? hv : rep_min(v, hv); f = f || hf; } }
    uint32_t run = rev ? rep_block_seg_excl<REP_SPINE_THREADS, true>(f, v, lds_f, lds_v)
                       : rep_block_seg_excl<REP_SPINE_THREADS, false>(f, v, lds_f, lds_v);
    if (!rev) {
        for (int64_t i = b; i < e; ++i) {
            carry[DOCREP_CARRY * i + dst] = run;
            const uint32_t hv = agg[DOCREP_AGG * i + src];
            run = agg[DOCREP_AGG * i] != 0 ? hv : rep_min(run, hv);
        }
    } else {
        for (int64_t i = e - 1; i >= b; --i) {
            carry[DOCREP_CARRY * i + dst] = run;
            const uint32_t hv = agg[DOCREP_AGG * i + src];
            run = agg[DOCREP_AGG * i] != 0 ? hv : rep_min(run, hv);
        }
    }
}

// Slots 1 + blockIdx.x * REP_TILE + threadIdx.x * REP_ITEMS + k.  mn (and, MODE ALL, mx) of the slot's whole run = what reaches
// it from the left joined with what reaches it from the right; a member that the rule of (MODE, SCOPE) flags: flag[SA[i]] = 1.
// Both are template parameters: KEEP_FIRST needs no maximum, so its instances drop two of the four block scans, and the scope
// picks the operands of two compares -- four small instances instead of branches inside the unrolled loops.
template <int MODE, int SCOPE>
__global__ __launch_bounds__(REP_THREADS) void k_docrep_mark(const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ lcps,
                                                              const uint32_t *__restrict__ dsv, const uint32_t *__restrict__ dev, uint32_t k_min,
                                                              const uint32_t *__restrict__ carry, uint8_t *__restrict__ flag)
{
    constexpr bool MAX = MODE == REP_MODE_ALL;
    __shared__ uint32_t lds_f[REP_WAVES], lds_v[REP_WAVES];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)t * REP_ITEMS + 1;
    uint32_t s[REP_ITEMS], ds[REP_ITEMS], de[REP_ITEMS], fw[REP_ITEMS], fx[REP_ITEMS];
    bool head[REP_ITEMS];
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const int64_t i = i0 + k;
        s[k] = i <= n ? SA[i] : REP_INF;
        head[k] = i <= n ? lcps[i - 1] < k_min : true;
        de[k] = i <= n ? dev[i - 1] : 0u;
        ds[k] = (SCOPE == DOCREP_OTHER && i <= n) ? dsv[i - 1] : 0u;
        if ((int64_t)s[k] >= n || de[k] == 0u) s[k] = REP_INF;       // not a member: the neutral element (a member's de is >= k_min >= 1)
    }
    // thread words: forward = (a head, minimum from the last head on), backward = (a head, minimum in front of the first head)
    bool any = false;
    uint32_t post = REP_INF, pre = REP_INF, postx = REP_INF, prex = REP_INF;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const uint32_t c = docrep_compl(s[k]);
        if (!any && !head[k]) { pre = rep_min(pre, s[k]); prex = rep_min(prex, c); }
        post = head[k] ? s[k] : rep_min(post, s[k]);
        postx = head[k] ? c : rep_min(postx, c);
        any = any || head[k];
    }
    const uint32_t *tc = carry + DOCREP_CARRY * (int64_t)blockIdx.x;
    const uint32_t tile_f = tc[0], tile_b = tc[1], tile_fx = MAX ? tc[2] : REP_INF, tile_bx = MAX ? tc[3] : REP_INF;
    if (t == 0 && !any) { post = rep_min(post, tile_f); postx = rep_min(postx, tile_fx); }
    if (t == REP_THREADS - 1 && !any) { pre = rep_min(pre, tile_b); prex = rep_min(prex, tile_bx); }
    const uint32_t cf = rep_block_seg_excl<REP_THREADS, false>(any, post, lds_f, lds_v);
    const uint32_t cb = rep_block_seg_excl<REP_THREADS, true>(any, pre, lds_f, lds_v);
    uint32_t cfx = REP_INF, cbx = REP_INF;
    if (MAX) {
        cfx = rep_block_seg_excl<REP_THREADS, false>(any, postx, lds_f, lds_v);
        cbx = rep_block_seg_excl<REP_THREADS, true>(any, prex, lds_f, lds_v);
    }
    uint32_t run = t == 0 ? tile_f : cf, runx = t == 0 ? tile_fx : cfx;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const uint32_t c = docrep_compl(s[k]);
        run = head[k] ? s[k] : rep_min(run, s[k]);
        runx = head[k] ? c : rep_min(runx, c);
        fw[k] = run; fx[k] = runx;
    }
    run = t == REP_THREADS - 1 ? tile_b : cb;
    runx = t == REP_THREADS - 1 ? tile_bx : cbx;
#pragma unroll
    for (int k = REP_ITEMS - 1; k >= 0; --k) {
        run = rep_min(run, s[k]);
        runx = rep_min(runx, docrep_compl(s[k]));
        if (s[k] != REP_INF) {
            const uint32_t mn = rep_min(run, fw[k]);
            const uint32_t mx = ~rep_min(runx, fx[k]);       // (no member besides position 0: 0)
            bool f;
            if (SCOPE == DOCREP_ANY) f = mn < s[k] || (MAX && mx > s[k]);
            else f = mn < ds[k] || (MAX && mx >= de[k]);
            if (f) flag[s[k]] = 1;
        }
        if (head[k]) { run = REP_INF; runx = REP_INF; }
    }
}

// Positions blockIdx.x * REP_TILE + threadIdx.x * REP_ITEMS + k.  flag, k_min, carry: what k_rep_spans<REP_MODE_KEEP_FIRST, .>
// takes (carry: the exclusive running maximum of the tiles' reach, still standing behind the span passes).  A position is
// covered iff the running maximum of the reach is above it.  The covered positions of document d are added to doc_bytes[d]
// (M - 1 entries, zeroed): once per workgroup when the tile's first and last position share a document, else once per wave
// when the wave's do, else once per thread when the thread's do, else once per run of positions of one document.
__global__ __launch_bounds__(REP_THREADS) void k_docrep_account(const uint8_t *__restrict__ flag, int64_t n, uint32_t k_min,
                                                                 const uint32_t *__restrict__ carry, const uint32_t *__restrict__ off, uint32_t M,
                                                                 uint32_t *__restrict__ doc_bytes)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    __shared__ uint32_t s_inc[REP_THREADS];
    __shared__ uint32_t s_d[2];
    const int t = threadIdx.x, l = lane_id();
    const int64_t tile0 = (int64_t)blockIdx.x * REP_TILE;
    const int64_t j0 = tile0 + (int64_t)t * REP_ITEMS;
    uint32_t x[REP_ITEMS];
    rep_load<REP_MODE_KEEP_FIRST>(flag, j0, n, k_min, x);
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) mx = mx > x[k] ? mx : x[k];
    uint32_t all;
    s_inc[t] = block_incl_max<REP_THREADS>(mx, lds, &all);
    __syncthreads();
    uint32_t run = carry[blockIdx.x];
    if (t) run = run > s_inc[t - 1] ? run : s_inc[t - 1];
    uint32_t bits = 0;                                       // bit k: position j0 + k is covered
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        const int64_t p = j0 + k;
        run = run > x[k] ? run : x[k];
        if (p < n && (int64_t)run > p) bits |= 1u << k;
    }
    const uint32_t cov = (uint32_t)__popc(bits);
    // the documents of the thread's first and last position (one search; the second only where the first document ends inside)
    const bool live = j0 < n;
    const int64_t jl = j0 + REP_ITEMS - 1 < n ? j0 + REP_ITEMS - 1 : n - 1;
    uint32_t d0 = DOC_NONE, d1 = DOC_NONE;
    if (live) {
        d0 = doc_lookup(off, M, (uint32_t)n, (uint32_t)j0);
        if (d0 >= M - 1) d0 = M - 2;                         // (never, for a sound table; keeps every index below inside it)
        d1 = (int64_t)off[d0 + 1] > jl ? d0 : doc_lookup(off, M, (uint32_t)n, (uint32_t)jl);
        if (d1 >= M - 1) d1 = M - 2;
    }
    const int64_t tile_last = (tile0 + REP_TILE < n ? tile0 + REP_TILE : n) - 1;
    if (t == 0) s_d[0] = d0;
    if (t == (int)((tile_last - tile0) / REP_ITEMS)) s_d[1] = d1;
    __syncthreads();
    if (s_d[0] == s_d[1]) {                                  // (block-uniform) the whole tile lies in one document
        uint32_t total;
        (void)block_excl_sum<REP_THREADS>(cov, lds, &total);
        if (t == 0 && total) atomicAdd(&doc_bytes[s_d[0]], total);
        return;
    }
    const unsigned long long lv = __ballot(live);            // live lanes are a prefix of the wave
    if (lv == 0) return;
    const uint32_t wd0 = (uint32_t)__shfl((int)d0, 0, WAVE);
    const uint32_t wd1 = (uint32_t)__shfl((int)d1, 63 - __clzll((long long)lv), WAVE);
    if (wd0 == wd1) {                                        // (wave-uniform) the wave's positions lie in one document
        uint32_t c = cov;
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
        if (l == 0 && c) atomicAdd(&doc_bytes[wd0], c);
        return;
    }
    if (!live) return;
    if (d0 == d1) {
        if (cov) atomicAdd(&doc_bytes[d0], cov);
        return;
    }
    uint32_t d = d0, c = 0;                                  // documents shorter than the thread's positions: one atomic per document
    for (int k = 0; k < REP_ITEMS; ++k) {
        const int64_t p = j0 + k;
        if (p >= n) break;
        while (d + 1 < M - 1 && (int64_t)off[d + 1] <= p) {
            if (c) atomicAdd(&doc_bytes[d], c);
            c = 0;
            ++d;
        }
        c += (bits >> k) & 1u;
    }
    if (c) atomicAdd(&doc_bytes[d], c);
}

// *dst += the number of documents with at least one covered byte
__global__ __launch_bounds__(REP_THREADS) void k_docrep_touched(const uint32_t *__restrict__ doc_bytes, int64_t ndocs, unsigned long long *__restrict__ dst)
{
    unsigned long long c = 0;
    for (int64_t d = (int64_t)blockIdx.x * REP_THREADS + threadIdx.x; d < ndocs; d += (int64_t)gridDim.x * REP_THREADS) c += doc_bytes[d] != 0u ? 1u : 0u;
    lcp_block_add(c, dst);
}

}  // namespace sa
