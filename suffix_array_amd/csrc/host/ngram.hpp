// host/ngram.hpp -- n-gram / infinity-gram queries over a device-resident index (kernels/ngram.hpp):
// sa_amd_index_next_bytes (the ranges by the search kernels, as host/docs.hpp gets them) and sa_amd_index_infgram (the ranges
// by the back-off kernel), then for both the continuations: count, one scan, ordered emission.  The steps of a query that do not
// depend on the alphabet are written once here; host/tokens.hpp orders them for the token index.
#pragma once
#include "docs.hpp"
#include "../kernels/ngram.hpp"

namespace sa {

static thread_local sa_amd_ngram_stats g_last_ngram_stats;
static thread_local int32_t g_ngram_stream_cap = -1;    // sa_amd_ngram_set_stream_cap of the calling thread (-1: NG_STREAM_CAP_DEFAULT)

// one wave per query, a wave takes every waves-th query: the counters cost one atomic per wave, not per query
static unsigned ngram_grid(int64_t queries)
{
    int64_t g = ceil_div(queries, NG_WAVES);
    const int64_t most = (int64_t)cu_count() * 16;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}

// ---- the steps that the byte queries (below) and the token queries (host/tokens.hpp) share; the two drivers order them ----

static int32_t ngram_stream_cap() { return g_ngram_stream_cap < 0 ? NG_STREAM_CAP_DEFAULT : g_ngram_stream_cap; }

// The fields that sa_amd_ngram_stats and sa_amd_tok_stats share, `compared` being compared_bytes / compared_tokens.  cw = the
// control words a call read back; nullptr: the state at the start of a call.
template <typename Stats>
static void ngram_stats_fill(Stats &s, int64_t &compared, int32_t count, bool backoff, const unsigned long long *cw, int passes, int readbacks)
{
    s.patterns = count;
    s.range_searches = !cw ? 0 : backoff ? (int64_t)cw[NG_W_SEARCHES] : (int64_t)count;
    compared = !backoff ? -1 : cw ? (int64_t)cw[NG_W_BYTES] : 0;
    s.stream_slots = cw ? (int64_t)cw[NG_W_STREAM_SLOTS] : 0;
    s.search_slots = cw ? (int64_t)cw[NG_W_SEARCH_SLOTS] : 0;
    s.stream_queries = cw ? (int64_t)cw[NG_W_STREAM_Q] : 0;
    s.search_queries = cw ? (int64_t)cw[NG_W_SEARCH_Q] : 0;
    s.empty_queries = cw ? (int64_t)cw[NG_W_EMPTY_Q] : 0;
    s.entries = cw ? (int64_t)cw[NG_W_TOTAL] : 0;
    s.stream_cap = ngram_stream_cap();
    s.readbacks = readbacks;
    s.backoff = backoff ? 1 : 0;
    s.passes = passes;
}

// The scratch of a call, at the start of its pooled block: control words, patterns, offsets, the listing's 8 bytes per query
// (nnz, then the scanned offsets), the scan's sums, and per query the range, the depth of the back-off and at_end.
struct NgScratch {
    unsigned long long *ctl = nullptr, *nnz = nullptr, *tsum = nullptr;
    void *pat = nullptr;
    int64_t *off = nullptr;
    uint32_t *lo = nullptr, *hi = nullptr, *len = nullptr;
    uint8_t *end = nullptr;
    const uint32_t *depth(bool backoff) const { return backoff ? len : nullptr; }
};

// Acquires the scratch and `more` bytes behind it, clears the control words and the listing's last count, and sends the
// patterns (symbols of `sym` bytes; pat_off counts symbols) and their offsets up.
static int ngram_begin(PooledScope &sc, NgScratch &s, const void *pat_data, const int64_t *pat_off, int32_t count, size_t sym, size_t more)
{
    const size_t C = (size_t)count, total = (size_t)pat_off[count] * sym;
    const size_t b_pat = align_up(total + 16, 256), b_off = align_up((C + 1) * 8, 256), b_w = align_up(C * 4 + 4, 256), b_b = align_up(C + 4, 256);
    const size_t b_ts = align_up(docs_scan_words((int64_t)C + 1) * 8, 256);
    sc.acquire(256 + b_pat + 2 * b_off + 3 * b_w + b_b + b_ts + more);
    s.ctl = (unsigned long long *)sc.take(256);
    s.pat = sc.take(b_pat);
    s.off = (int64_t *)sc.take(b_off);
    s.nnz = (unsigned long long *)sc.take(b_off); s.tsum = (unsigned long long *)sc.take(b_ts);
    s.lo = (uint32_t *)sc.take(b_w); s.hi = (uint32_t *)sc.take(b_w); s.len = (uint32_t *)sc.take(b_w);
    s.end = (uint8_t *)sc.take(b_b);
    if (sc.rc) return sc.rc;
    HIP_TRY(hipMemsetAsync(s.ctl, 0, 256, sc.st));
    HIP_TRY(hipMemsetAsync(s.nnz + C, 0, 8, sc.st));
    if (total) HIP_TRY(hipMemcpyAsync(s.pat, pat_data, total, hipMemcpyHostToDevice, sc.st));
    HIP_TRY(hipMemcpyAsync(s.off, pat_off, (C + 1) * 8, hipMemcpyHostToDevice, sc.st));
    return SA_AMD_OK;
}

// One run of a continuation kernel (k_next_bytes / k_tok_next, <false> or <true>) over the ranges in the scratch
template <typename Kernel, typename Sym>
static int ngram_pass(Kernel kernel, const Sym *T, const uint32_t *SA, int32_t n, const NgScratch &s, bool backoff, int32_t count, uint8_t *at_end,
                       Sym *syms, uint32_t *counts, size_t cap, hipStream_t st)
{
    PROF(KC_MISC, count, st, hipLaunchKernelGGL(kernel, dim3(ngram_grid(count)), dim3(NG_THREADS), 0, st, T, SA, (int64_t)n, (const uint32_t *)s.lo,
                                                (const uint32_t *)s.hi, s.depth(backoff), (const int64_t *)s.off, count, (uint32_t)ngram_stream_cap(), at_end,
                                                s.nnz, syms, counts, (unsigned long long)cap, s.ctl));
    return SA_AMD_OK;
}

// The counting pass and the scan of its counts: nnz becomes the listing's offsets, ctl[NG_W_TOTAL] its length
template <typename Kernel, typename Sym>
static int ngram_count(Kernel count_kernel, const Sym *T, const uint32_t *SA, int32_t n, const NgScratch &s, bool backoff, int32_t count, hipStream_t st)
{
    { const int rcp = ngram_pass(count_kernel, T, SA, n, s, backoff, count, s.end, (Sym *)nullptr, (uint32_t *)nullptr, 0, st); if (rcp) return rcp; }
    return docs_scan(s.nnz, (int64_t)count + 1, s.tsum, &s.ctl[NG_W_TOTAL], st);
}

// the per-query outputs and the listing's offsets, straight into the caller's arrays
static void ngram_down(PooledScope &sc, const NgScratch &s, int32_t count, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi,
                       uint8_t *at_end, int64_t *list_off)
{
    const size_t C = (size_t)count;
    if (suffix_len) sc.down(suffix_len, s.len, C * 4);
    if (range_lo) sc.down(range_lo, s.lo, C * 4);
    if (range_hi) sc.down(range_hi, s.hi, C * 4);
    if (at_end) sc.down(at_end, s.end, C);
    if (list_off) sc.down(list_off, s.nnz, (C + 1) * 8);
}

// backoff == false: sa_amd_index_next_bytes (suffix_len is nullptr).  backoff == true: sa_amd_index_infgram.  Host pointers,
// every output may be nullptr, arguments checked by the caller.  All scratch is one pooled block: 8 bytes per query for the
// listing (the continuations are computed twice -- counted, then emitted -- instead of kept at 1 KiB per query), and the
// device side of the listing, min(capacity, 256 count) entries, so the emission is queued before the one blocking read-back:
// the listing's length and the counters.
static int ngram_query(const sa_amd_index &ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, bool backoff, int32_t min_count,
                       int32_t max_len, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end, int64_t *list_off,
                       uint8_t *bytes, uint32_t *counts, int64_t capacity, int64_t *total_out)
{
    sa_amd_ngram_stats ns;
    memset(&ns, 0, sizeof(ns));
    ngram_stats_fill(ns, ns.compared_bytes, count, backoff, nullptr, 0, 0);
    g_last_ngram_stats = ns;
    if (count == 0) {
        if (list_off) list_off[0] = 0;
        if (total_out) *total_out = 0;
        return SA_AMD_OK;
    }
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const int rb0 = g_readbacks;
    const int64_t most = 256 * (int64_t)count;
    const size_t cap = bytes || counts ? (size_t)(capacity < most ? capacity : most) : 0;

    PooledScope sc(ix.device, false);
    NgScratch s;
    const size_t b_lb = align_up(cap + 8, 256), b_lc = align_up(cap * 4 + 8, 256);
    { const int rcb = ngram_begin(sc, s, pat_data, pat_off, count, 1, b_lb + b_lc); if (rcb) return rcb; }
    uint8_t *dBytes = (uint8_t *)sc.take(b_lb);
    uint32_t *dCounts = (uint32_t *)sc.take(b_lc);
    if (sc.rc) return sc.rc;
    hipStream_t st = sc.st;

    // ---- the ranges: the search kernels as sa_amd_index_search runs them, or the back-off ----
    if (backoff) {
        PROF(KC_MISC, count, st, hipLaunchKernelGGL((k_infgram_suffix<uint8_t>), dim3(ngram_grid(count)), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(),
                                                    (int64_t)ix.n, ix.bkt(), ix.pair(), esa_log_p(ix.n), (const uint8_t *)s.pat, (const int64_t *)s.off, count,
                                                    (uint32_t)min_count, (int64_t)max_len, s.len, s.lo, s.hi, s.ctl));
    } else {
        g_prof.begin(KC_MISC, count, st);
        const int rcs = launch_search(ix.text(), ix.sa(), ix.n, ix.bkt(), ix.pair(), (const uint8_t *)s.pat, s.off, count, nullptr, s.lo, s.hi, nullptr,
                                      nullptr, nullptr, st);
        g_prof.end(st);
        if (rcs) return rcs;
    }
    // ---- the continuations: counted, scanned, emitted in order ----
    { const int rcn = ngram_count(k_next_bytes<false>, ix.text(), ix.sa(), ix.n, s, backoff, count, st); if (rcn) return rcn; }
    if (cap > 0) {
        const int rce = ngram_pass(k_next_bytes<true>, ix.text(), ix.sa(), ix.n, s, backoff, count, nullptr, bytes ? dBytes : nullptr,
                                   counts ? dCounts : nullptr, cap, st);
        if (rce) return rce;
    }
    unsigned long long cw[NG_W_COUNT];
    { const int rcw = read_words(cw, s.ctl, sizeof(cw), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t listed = (int64_t)cw[NG_W_TOTAL];
    if (listed < 0 || listed > most) return SA_AMD_EINTERNAL;
    const size_t wr = (size_t)listed < cap ? (size_t)listed : cap;

    // ---- down: straight into the caller's arrays ----
    if (bytes && wr > 0) sc.down(bytes, dBytes, wr);
    if (counts && wr > 0) sc.down(counts, dCounts, wr * 4);
    ngram_down(sc, s, count, suffix_len, range_lo, range_hi, at_end, list_off);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    if (total_out) *total_out = listed;
    g_prof.resolve();
    ngram_stats_fill(ns, ns.compared_bytes, count, backoff, cw, cap > 0 ? 2 : 1, g_readbacks - rb0);
    g_last_ngram_stats = ns;
    return SA_AMD_OK;
}

}  // namespace sa
