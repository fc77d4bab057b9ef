// kernels/ngram.hpp -- n-gram / infinity-gram queries over the device index: the longest suffix of a
// prompt that occurs at least min_count times (k_infgram_suffix: a bisection on the suffix length, every probe one range
// search) and, for a match range [lo, hi) of a context of p bytes, the counts of the byte that follows it (k_next_bytes).
// Inside the range the slots are sorted by T[SA[i] + p], so the 256 counts are the places of at most 256 run starts: found by
// streaming the range once (short ranges) or by binary searches between 64 samples (long ones).  One wave per query, no
// atomics on the answers.  gfx950, wave64.  Every slot read lies in [0, n + 1) and every SA entry is checked against n before
// T is read through it, whatever the arrays hold.
#pragma once
#include "sym.hpp"
#include "esa.hpp"
#include "docs.hpp"

namespace sa {

constexpr int NG_THREADS = 256;
constexpr int NG_WAVES = NG_THREADS / WAVE;
constexpr int NG_LOADS = 4;                        // slots a lane of the streaming route has in flight
constexpr int NG_STREAM_CAP_DEFAULT = 1024;        // sa_amd_ngram_set_stream_cap
constexpr int NG_STREAM_CAP_MAX = 0x7fffffff;      // (no range is longer: n + 1 < 2^31)
constexpr int NG_END = 256;                        // the "byte" of a slot whose suffix ends at the context: sym_end<uint8_t>()
constexpr uint32_t NG_NONE = 0xffffffffu;          // a byte value without a run

// the control words of a call (unsigned long long each)
enum { NG_W_TOTAL = 0, NG_W_SEARCHES, NG_W_BYTES, NG_W_STREAM_SLOTS, NG_W_SEARCH_SLOTS, NG_W_STREAM_Q, NG_W_SEARCH_Q, NG_W_EMPTY_Q, NG_W_COUNT };

// The match range of pat[0 .. plen) as the search kernels report it: over the pair table the left ends of the two descents of
// k_esa_search, without it plain_range (kernels/sym.hpp), narrowed by the bucket table where there is one.  Both tables are
// byte-only: for any other Sym those branches are compiled out and the caller passes nullptr, nullptr, 0.  Executed by a whole
// wave; *symbols grows by the text symbols compared.
template <typename Sym>
__device__ __forceinline__ NgRange ngram_range(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n,
                                               const uint32_t *__restrict__ bkt, const uint64_t *__restrict__ pair, int log_p,
                                               const Sym *__restrict__ pat, int64_t plen, int64_t *symbols)
{
    int64_t lo = 0, hi = n + 1;
    if constexpr (std::is_same<Sym, uint8_t>::value) {
        if (pair) {
            int64_t table_steps = 0;
            const EsaState a = esa_descent<false>(T, SA, n, pair, log_p, pat, plen, symbols, &table_steps);
            const EsaState b = esa_descent<true>(T, SA, n, pair, log_p, pat, plen, symbols, &table_steps);
            NgRange r;
            r.lo = (uint32_t)a.L; r.hi = (uint32_t)b.L;
            return r;
        }
        if (bkt && plen > 1) {
            const int idx = (int)pat[0] * 257 + (int)pat[1] + 2;
            lo = bkt[idx - 1]; hi = bkt[idx];
        } else if (bkt && plen == 1) {
            lo = bkt[(int)pat[0] * 257]; hi = bkt[(int)pat[0] * 257 + 257];
        }
    }
    return plain_range(T, SA, n, lo, hi, pat, plen, symbols);
}

// Back-off.  Prompt q has L symbols and cap = L, or min(L, max_len) with max_len > 0.  The count of its suffix of s symbols never
// grows with s, s = 0 (range [0, n + 1)) always qualifies and cap + 1 stands for "does not": the bisection keeps
// good < bad, probes s = (good + bad) / 2 with one range search of P + L - s and ends after at most ceil(log2(cap + 1)) probes.
// suffix_len / range_lo / range_hi: the largest qualifying s and its range.  ctl[NG_W_SEARCHES] += probes, ctl[NG_W_BYTES] +=
// text symbols compared (one atomic per wave each, behind all of the wave's prompts).
template <typename Sym>
__global__ __launch_bounds__(NG_THREADS) void k_infgram_suffix(
    const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ bkt,
    const uint64_t *__restrict__ pair, int log_p, const Sym *__restrict__ pat_data, const int64_t *__restrict__ pat_off, int32_t count,
    uint32_t min_count, int64_t max_len, uint32_t *__restrict__ suffix_len, uint32_t *__restrict__ range_lo, uint32_t *__restrict__ range_hi,
    unsigned long long *__restrict__ ctl)
{
    const int64_t waves = (int64_t)gridDim.x * NG_WAVES;
    int64_t symbols = 0, searches = 0;
    for (int64_t q = (int64_t)blockIdx.x * NG_WAVES + wave_id(); q < count; q += waves) {
        const Sym *pat = pat_data + pat_off[q];
        const int64_t L = pat_off[q + 1] - pat_off[q];
        const int64_t cap = max_len > 0 && max_len < L ? max_len : L;
        int64_t good = 0, bad = cap + 1;
        uint32_t lo = 0, hi = (uint32_t)n + 1u;
        while (bad - good > 1) {
            const int64_t s = good + (bad - good) / 2;
            const NgRange r = ngram_range(T, SA, n, bkt, pair, log_p, pat + (L - s), s, &symbols);
            ++searches;
            if (r.hi > r.lo && r.hi - r.lo >= min_count) { good = s; lo = r.lo; hi = r.hi; } else bad = s;
        }
        if (lane_id() == 0) { suffix_len[q] = (uint32_t)good; range_lo[q] = lo; range_hi[q] = hi; }
    }
    if (lane_id() == 0) {
        if (searches) atomicAdd(&ctl[NG_W_SEARCHES], (unsigned long long)searches);
        if (symbols) atomicAdd(&ctl[NG_W_BYTES], (unsigned long long)symbols);
    }
}

// ---- the front and back that the two continuation kernels (k_next_bytes, k_tok_next of kernels/tokens.hpp) share ----

// The window of query q: its range [lo, hi) clamped to the n + 1 slots, the depth p (depth[q], or the pattern's length where
// depth is nullptr), and ae = the range's first slot ends at the context; that slot is stripped: s0 = lo + ae, cnt = hi - s0.
struct NgWindow { uint32_t s0, cnt, ae; int64_t p; };

__device__ __forceinline__ NgWindow ng_window(const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ range_lo,
                                              const uint32_t *__restrict__ range_hi, const uint32_t *__restrict__ depth,
                                              const int64_t *__restrict__ pat_off, int64_t q)
{
    const uint32_t N1 = (uint32_t)n + 1u;
    uint32_t hi = range_hi[q], lo = range_lo[q];
    if (hi > N1) hi = N1;
    if (lo > hi) lo = hi;
    NgWindow w;
    w.p = depth ? (int64_t)depth[q] : pat_off[q + 1] - pat_off[q];
    w.ae = hi > lo && (int64_t)SA[lo] + w.p >= n ? 1u : 0u;
    w.s0 = lo + w.ae; w.cnt = hi - w.s0;
    return w;
}

// One trip of the streaming route: b[t] = the symbol behind the context of place r + 64 t + lane (sym_end past cnt or where the
// suffix ends), NG_LOADS * 64 places.  The slot loads come first, then the symbol loads: all loads of a trip are in flight together.
template <typename Sym>
__device__ __forceinline__ void ng_stream_trip(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const NgWindow &w,
                                               uint32_t r, int b[NG_LOADS])
{
    uint32_t s[NG_LOADS];
#pragma unroll
    for (int t = 0; t < NG_LOADS; ++t) {
        const uint32_t i = r + (uint32_t)t * WAVE + lane_id();
        s[t] = i < w.cnt ? SA[w.s0 + i] : 0xffffffffu;
    }
#pragma unroll
    for (int t = 0; t < NG_LOADS; ++t) {
        const int64_t at = (int64_t)s[t] + w.p;                           // (an unread slot: 2^32 - 1 + p >= n)
        b[t] = at < n ? (int)T[at] : sym_end<Sym>();
    }
}

// The searching route's 64 samples: lane l probes place pos = l (cnt - 1) / 63 and gets its symbol b; posn and bn are those of
// the next lane.  The run that starts the range (place 0, lane 0's b) is the caller's.
struct NgSample { uint32_t pos, posn; int b, bn; };

template <typename Sym>
__device__ __forceinline__ NgSample ng_sample(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const NgWindow &w)
{
    NgSample s;
    s.pos = (uint32_t)(((uint64_t)lane_id() * (w.cnt - 1)) / (WAVE - 1));
    s.b = next_symbol(T, SA, n, w.p, w.s0 + s.pos);
    s.bn = __shfl_down(s.b, 1, WAVE);
    s.posn = (uint32_t)__shfl_down((int)s.pos, 1, WAVE);
    return s;
}

// The boundary walk between a lane's sample and the next: where the sample's symbol is below the next one's, run starts lie
// between them, and the lane finds each by a binary search for the first place with a symbol above the last one found -- the
// upper end of the search is always a probed place, so the symbol of the start is known without another probe.  found(place,
// symbol) is called once per run start, in ascending order; returns the probes made.
template <typename Sym, typename Found>
__device__ __forceinline__ uint32_t ng_walk(const Sym *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const NgWindow &w,
                                            const NgSample &s, Found &&found)
{
    uint32_t probes = 0;
    if (lane_id() < WAVE - 1) {
        int x = s.b;
        uint32_t a = s.pos;
        while (x < s.bn) {                                                // a run starts in (a, posn]: symbol(posn) = bn > x
            uint32_t u = a + 1, v = s.posn;
            int bv = s.bn;                                                // the symbol of place v, always a probed one
            while (u < v) {
                const uint32_t m = u + (v - u) / 2;
                const int bm = next_symbol(T, SA, n, w.p, w.s0 + m);
                ++probes;
                if (bm > x) { v = m; bv = bm; } else u = m + 1;
            }
            found(u, bv);
            x = bv; a = u;
        }
    }
    return probes;
}

// the counters of a wave over all of its queries, and their flush: one atomic per wave and counter
struct NgCounters { unsigned long long stream_slots = 0, search_slots = 0; uint32_t stream_q = 0, search_q = 0, empty_q = 0; };

__device__ __forceinline__ void ng_flush(const NgCounters &c, unsigned long long *__restrict__ ctl)
{
    const int l = lane_id();
    if (l == WAVE - 1 && c.search_slots) atomicAdd(&ctl[NG_W_SEARCH_SLOTS], c.search_slots);       // (wave_incl_sum: lane 63 holds the sum)
    if (l == 0) {
        if (c.stream_slots) atomicAdd(&ctl[NG_W_STREAM_SLOTS], c.stream_slots);
        if (c.stream_q) atomicAdd(&ctl[NG_W_STREAM_Q], (unsigned long long)c.stream_q);
        if (c.search_q) atomicAdd(&ctl[NG_W_SEARCH_Q], (unsigned long long)c.search_q);
        if (c.empty_q) atomicAdd(&ctl[NG_W_EMPTY_Q], (unsigned long long)c.empty_q);
    }
}

// Continuations of query q over its window (ng_window).
// The wave fills a table in LDS with the place, relative to s0, where the run of every byte value starts (NG_NONE: no run;
// entry 256 = cnt, the end of the last run):
//   cnt <= stream_cap: the range is read once, NG_LOADS * 64 slots a trip; a lane compares its byte with its left neighbour's
//     (a shuffle; the last byte of a trip is carried into the next) and stores its place where they differ.  cnt slots probed.
//   else: the 64 samples and the walk between them (ng_sample, ng_walk).  At most 64 + 255 ceil(log2 cnt) slots probed.
// Then lane l holds byte values 4 l .. 4 l + 3: the count of a present value is the next present start less its own.
// EMIT = false: nnz[q] = the number of non-zero counts (nnz[count] is the host's), at_end[q], and the counters -- one atomic per
// wave each behind all of its queries.  EMIT = true: nnz holds the scanned offsets; the non-zero (byte, count) pairs go to
// bytes / counts (either may be nullptr) in ascending byte order from nnz[q] on, while the offset is below `capacity`.
template <bool EMIT>
__global__ __launch_bounds__(NG_THREADS) void k_next_bytes(
    const uint8_t *__restrict__ T, const uint32_t *__restrict__ SA, int64_t n, const uint32_t *__restrict__ range_lo,
    const uint32_t *__restrict__ range_hi, const uint32_t *__restrict__ depth, const int64_t *__restrict__ pat_off, int32_t count,
    uint32_t stream_cap, uint8_t *__restrict__ at_end, unsigned long long *__restrict__ nnz, uint8_t *__restrict__ bytes,
    uint32_t *__restrict__ counts, unsigned long long capacity, unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t s_start[NG_WAVES][NG_END + 1];
    uint32_t *start = s_start[wave_id()];
    const int l = lane_id();
    const int64_t waves = (int64_t)gridDim.x * NG_WAVES;
    NgCounters ctr;
    for (int64_t q = (int64_t)blockIdx.x * NG_WAVES + wave_id(); q < count; q += waves) {
        const NgWindow w = ng_window(SA, n, range_lo, range_hi, depth, pat_off, q);
        const uint32_t cnt = w.cnt, ae = w.ae;
        for (int b = l; b <= NG_END; b += WAVE) start[b] = b == NG_END ? cnt : NG_NONE;
        if (cnt == 0) {
            ++ctr.empty_q;
        } else if (cnt <= stream_cap) {
            ++ctr.stream_q;
            ctr.stream_slots += cnt;
            int carry = -1;
            for (uint32_t r = 0; r < cnt; r += NG_LOADS * WAVE) {
                int b[NG_LOADS];
                ng_stream_trip(T, SA, n, w, r, b);
#pragma unroll
                for (int t = 0; t < NG_LOADS; ++t) {
                    const uint32_t i = r + (uint32_t)t * WAVE + l;
                    int left = __shfl_up(b[t], 1, WAVE);
                    if (l == 0) left = carry;
                    if (i < cnt && b[t] != left && b[t] < NG_END) start[b[t]] = i;
                    carry = __shfl(b[t], WAVE - 1, WAVE);
                }
            }
        } else {
            ++ctr.search_q;
            const NgSample smp = ng_sample(T, SA, n, w);
            if (l == 0 && smp.b < NG_END) start[smp.b] = 0;
            const uint32_t probes = 1 + ng_walk(T, SA, n, w, smp, [&](uint32_t u, int bv) { if (bv < NG_END) start[bv] = u; });
            ctr.search_slots += wave_incl_sum(probes);                    // (lane 63 holds the wave's sum)
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // the wave's own LDS stores have landed
        uint32_t v[4], c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = start[4 * l + k];
        uint32_t sm = v[0];                                               // NG_NONE is the largest value: min skips the absent
#pragma unroll
        for (int k = 1; k < 4; ++k) sm = v[k] < sm ? v[k] : sm;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {                              // inclusive suffix minimum over the lanes
            const uint32_t t = (uint32_t)__shfl_down((int)sm, o, WAVE);
            if (l + o < WAVE && t < sm) sm = t;
        }
        uint32_t nx = (uint32_t)__shfl_down((int)sm, 1, WAVE);            // the next present start behind this lane's values
        const uint32_t endv = start[NG_END];
        if (l == WAVE - 1 || nx > endv) nx = endv;
        uint32_t nz = 0;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            c[k] = v[k] != NG_NONE && nx > v[k] ? nx - v[k] : 0u;
            if (v[k] != NG_NONE) nx = v[k];
            nz += c[k] ? 1u : 0u;
        }
        const uint32_t incl = wave_incl_sum(nz);
        if (!EMIT) {
            if (l == WAVE - 1) { nnz[q] = incl; at_end[q] = (uint8_t)ae; }
        } else {
            unsigned long long o = nnz[q] + (incl - nz);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!c[k]) continue;
                if (o < capacity) {
                    if (bytes) bytes[o] = (uint8_t)(4 * l + k);
                    if (counts) counts[o] = c[k];
                }
                ++o;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // the table is read before the next query fills it
    }
    if (!EMIT) ng_flush(ctr, ctl);
}

static_assert(NG_END == sym_end<uint8_t>(), "NG_END is the byte alphabet's sentinel");

}  // namespace sa
