// host/tokens.hpp -- texts over a token alphabet (kernels/tokens.hpp): 16-bit tokens and token ids below
// 2^24 in uint32_t (section 25).  Everything is written once over the token type Sym: the type behind the ABI's
// `sa_amd_tok_index *` / `sa_amd_tok32_index *` (the owner of the token text and its suffix array, as host/index.hpp is for the
// byte index), the token build -- byte image, the byte builder on it, compaction -- behind sa_amd_saca_u16 / _u32 and the two
// index_create, and the queries: _search, _next_tokens and _infgram.  The two _infgram_score are host/score.hpp's route on these
// index types.  A token index owns a document collection as the byte index does: the document routes of
// host/docs.hpp and host/doc_match.hpp run on it through the range step below, and tok_docs_by_separator defines the collection
// from the resident text.
#pragma once
#include "ngram.hpp"
#include "doc_match.hpp"
#include "../../../include/sa_amd_tokdocs.h"
#include "../kernels/tokens.hpp"

namespace sa {

// Token text (n tokens, 16 bytes of slack behind them) and token suffix array (n + 1 entries) kept in HBM.  Both are DevBufs of
// the index's own: deleting the index frees them, in no call that can throw and without a change of device.
template <typename SymT>
struct TokIndexOwner {
    using Sym = SymT;
    int device = 0;
    int32_t n = 0;
    uint32_t ndocs = 0;
    DevBuf dT, dSA;
    DevBuf dDocOff;        // document offsets in tokens (ndocs + 1 entries) once a _set_documents call has taken a collection
    DevBuf dDocPrev;       // per slot: the previous slot of the same document + 1 (n + 1 entries)
    const Sym *text() const { return dT.as<const Sym>(); }
    const uint32_t *sa() const { return dSA.as<const uint32_t>(); }
    const uint32_t *doc_off() const { return dDocOff.as<const uint32_t>(); }
    const uint32_t *doc_prev() const { return dDocPrev.as<const uint32_t>(); }
    // no bucket table and no LCP table: what the index-generic routes (host/score.hpp) pass to the kernels
    const uint32_t *bkt() const { return nullptr; }
    const uint64_t *pair() const { return nullptr; }
};

}  // namespace sa

extern "C++" {

struct sa_amd_tok_index : sa::TokIndexOwner<uint16_t> { };
struct sa_amd_tok32_index : sa::TokIndexOwner<uint32_t> { };

}  // extern "C++"

namespace sa {

constexpr int32_t TOK_MAX_TOKENS_U16 = SA_AMD_MAX_LENGTH / 2;      // the byte image has 2 n <= 2^31 - 2 bytes
constexpr int32_t TOK_MAX_TOKENS_U32 = SA_AMD_MAX_LENGTH / 3;      // the byte image has 3 n <= 2^31 - 1 bytes
static_assert(SA_AMD_TOKEN_LIMIT_U32 == TK_LIMIT_U32, "the header's limit is the kernels'");

static thread_local sa_amd_tok_stats g_last_tok_stats;

static unsigned tok_stream_grid(int64_t items, int per_block)
{
    int64_t g = ceil_div(items, per_block);
    const int64_t most = (int64_t)cu_count() * 8;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}

// The scratch of one token build, carved from the scope's block in this order: the byte builder's work block, the byte image,
// the byte-level array, and (32-bit tokens) the range flag.  Once the builder is done its work block holds the compaction's
// output (where the caller has no buffer of its own for it) and, behind that, the tile counts and the scan's tile sums.
struct TokBuild {
    size_t wb = 0, b_out = 0, b_cnt = 0, b_img = 0, b_sa2 = 0, b_flag = 0;
    int64_t tiles = 0;
    size_t bytes() const { return wb + b_img + b_sa2 + b_flag; }
};

template <typename Sym>
static TokBuild tok_build_layout(int32_t n)
{
    constexpr int64_t stride = TokStrideOf<Sym>::value;
    TokBuild L;
    const int64_t len = stride * (int64_t)n + 1;
    L.tiles = ceil_div(len, TK_TILE);
    L.b_out = align_up(((size_t)n + 1) * 4, 256);
    L.b_cnt = align_up((size_t)(L.tiles + 1) * 8, 256);
    const size_t after = L.b_out + L.b_cnt + align_up(docs_scan_words(L.tiles + 1) * 8, 256);
    L.wb = align_up((size_t)carve(nullptr, stride * (int64_t)n).bytes, 256);
    if (L.wb < after) L.wb = after;
    L.b_img = align_up((size_t)(stride * n) + 16, 256);
    L.b_sa2 = align_up((size_t)len * 4, 256);
    L.b_flag = sizeof(Sym) == 4 ? 256 : 0;
    return L;
}

// The token suffix array (n + 1 entries) of dT[0 .. n), n > 0 (device pointers, dT 16-byte aligned with 16 bytes of slack
// behind the tokens) -> dOut, or, dOut == nullptr, the start of the work block; *out_ptr: where it is.  The scope has acquired
// at least L.bytes() more than has been taken.  Blocks until done; the three times go to the calling thread's statistics.
// 32-bit tokens: the image pass raises the range flag, which is read where the stream is drained for image_ms -- before the byte
// builder starts; an id of 2^24 or more is SA_AMD_ERANGE with nothing built.
template <typename Sym>
static int32_t tok_build_device(PooledScope &sc, const TokBuild &L, const Sym *dT, int32_t n32, uint32_t *dOut, const uint32_t **out_ptr)
{
    constexpr int stride = TokStrideOf<Sym>::value;
    const int64_t n = n32, len = stride * n + 1;
    char *dW = (char *)sc.take(L.wb);
    uint8_t *dB = (uint8_t *)sc.take(L.b_img);
    uint32_t *dSA2 = (uint32_t *)sc.take(L.b_sa2);
    uint32_t *flags = L.b_flag ? (uint32_t *)sc.take(L.b_flag) : nullptr;
    if (sc.rc) return sc.rc;
    hipStream_t st = sc.st;
    double t0 = now_ms();
    if constexpr (stride == 2) {
        PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_tok_be_image, dim3(tok_stream_grid(ceil_div(n, TK_IMAGE_ITEMS), TK_THREADS)), dim3(TK_THREADS), 0, st,
                                                dT, dB, n));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        HIP_TRY(hipMemsetAsync(flags, 0, 4, st));
        PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_tok_be_image3, dim3(tok_stream_grid(ceil_div(n, TK_IMAGE3_ITEMS), TK_THREADS)), dim3(TK_THREADS), 0, st,
                                                dT, dB, n, flags));
        uint32_t f = 0;
        { const int rcw = read_words(&f, flags, 4, st); if (rcw) return rcw; }
        HIP_TRY(hipStreamSynchronize(st));
        if (f & 1u) return SA_AMD_ERANGE;
    }
    double t1 = now_ms();
    g_last_tok_stats.image_ms = t1 - t0;
    { const int rcb = build_device(dB, dSA2, (int32_t)(stride * n), dW, (int64_t)L.wb, st, nullptr); if (rcb) return rcb; }
    t0 = now_ms();
    g_last_tok_stats.build_ms = t0 - t1;
    // ---- the entries divisible by the stride, divided by it, in their order: tile counts, one scan, scatter ----
    if (!dOut) dOut = (uint32_t *)dW;
    unsigned long long *cnt = (unsigned long long *)(dW + L.b_out), *tsum = (unsigned long long *)(dW + L.b_out + L.b_cnt);
    const unsigned grid = tok_stream_grid(ceil_div(L.tiles, TK_SPAN), 1);
    PROF(KC_MISC, len, st, hipLaunchKernelGGL(k_tok_compact_count, dim3(grid), dim3(TK_THREADS), 0, st, (const uint32_t *)dSA2, len, L.tiles, cnt,
                                              TokStride<stride>()));
    { const int rcs = docs_scan(cnt, L.tiles + 1, tsum, nullptr, st); if (rcs) return rcs; }
    PROF(KC_MISC, len, st, hipLaunchKernelGGL(k_tok_compact_scatter, dim3(grid), dim3(TK_THREADS), 0, st, (const uint32_t *)dSA2, len, L.tiles,
                                              (const unsigned long long *)cnt, dOut, n + 1, TokStride<stride>()));
    HIP_TRY(hipStreamSynchronize(st));
    g_last_tok_stats.compact_ms = now_ms() - t0;
    g_prof.resolve();
    if (out_ptr) *out_ptr = dOut;
    return SA_AMD_OK;
}

// sa_amd_saca_u16 / sa_amd_saca_u32 behind their argument checks, n > 0: one pooled block -- T | the build's scratch --, only
// the final array comes down (nothing where the build failed)
template <typename Sym>
static int32_t tok_saca_host(const Sym *T, uint32_t *SA, int32_t n)
{
    PooledScope sc(pick_device(), false);
    const TokBuild L = tok_build_layout<Sym>(n);
    const size_t b_t = align_up(sizeof(Sym) * (size_t)n + 16, 256);
    sc.acquire(b_t + L.bytes());
    Sym *dT = (Sym *)sc.take(b_t);
    if (sc.rc) return sc.rc;
    HIP_TRY(hipMemcpyAsync(dT, T, sizeof(Sym) * (size_t)n, hipMemcpyHostToDevice, sc.st));
    const uint32_t *dOut = nullptr;
    sc.rc = tok_build_device(sc, L, dT, n, nullptr, &dOut);
    sc.down(SA, dOut, ((size_t)n + 1) * 4);
    return sc.finish();
}

// sa_amd_tok_index_create / sa_amd_tok32_index_create behind their argument checks: the tokens go up, and the caller's array
// (range-checked before anything reads through it; 32-bit tokens: so is the text, in the same flag) or, SA == nullptr, the one
// built on the device; *out owns both
template <typename Index>
static int32_t tok_index_create(const typename Index::Sym *T, int32_t n, const uint32_t *SA, Index **out)
{
    using Sym = typename Index::Sym;
    DeviceGuard guard(pick_device());
    if (guard.rc != SA_AMD_OK) return guard.rc;
    DevBuf dT, dSA;
    const size_t N = (size_t)n;
    if (index_table_alloc(dT, sizeof(Sym) * N + 16) != SA_AMD_OK || index_table_alloc(dSA, (N + 1) * 4) != SA_AMD_OK) return SA_AMD_ENOMEM;
    if (N) HIP_TRY(hipMemcpy(dT.p, T, sizeof(Sym) * N, hipMemcpyHostToDevice));
    if (SA) {
        PooledScope sc(-1, false);
        sc.acquire(256);
        uint32_t *flags = (uint32_t *)sc.take(256);
        if (sc.rc) return sc.rc;
        HIP_TRY(hipMemcpyAsync(dSA.p, SA, (N + 1) * 4, hipMemcpyHostToDevice, sc.st));
        HIP_TRY(hipMemsetAsync(flags, 0, 4, sc.st));
        PROF(KC_MISC, n, sc.st, hipLaunchKernelGGL(k_tok_sa_range, dim3(tok_stream_grid((int64_t)n + 1, TK_THREADS)), dim3(TK_THREADS), 0, sc.st,
                                                   dSA.as<const uint32_t>(), (int64_t)n, flags));
        if constexpr (sizeof(Sym) == 4)
            PROF(KC_MISC, n, sc.st, hipLaunchKernelGGL(k_tok_id_range, dim3(tok_stream_grid((int64_t)n, TK_THREADS)), dim3(TK_THREADS), 0, sc.st,
                                                       dT.as<const uint32_t>(), (int64_t)n, flags));
        uint32_t f = 0;
        { const int rcw = read_words(&f, flags, 4, sc.st); if (rcw) return rcw; }
        if (sc.finish() != SA_AMD_OK) return sc.rc;
        if (f & 1u) return SA_AMD_ERANGE;
        if (SA[0] != (uint32_t)n) return SA_AMD_EINVAL;
    } else if (n == 0) {
        HIP_TRY(hipMemset(dSA.p, 0, 4));
    } else {
        PooledScope sc(-1, false);
        const TokBuild L = tok_build_layout<Sym>(n);
        sc.acquire(L.bytes());
        sc.rc = sc.rc ? sc.rc : tok_build_device(sc, L, dT.as<const Sym>(), n, dSA.as<uint32_t>(), nullptr);
        if (sc.finish() != SA_AMD_OK) return sc.rc;
    }
    Index *ix = new (std::nothrow) Index();
    if (!ix) return SA_AMD_ENOMEM;
    ix->n = n;
    (void)hipGetDevice(&ix->device);
    ix->dT = std::move(dT);
    ix->dSA = std::move(dSA);
    *out = ix;
    return SA_AMD_OK;
}

// ---- document collections (host/docs.hpp, host/doc_match.hpp): what the token index supplies to the shared routes ----

// the range step: k_tok_search as _search runs it, no bucket table and no LCP table; dO counts tokens
template <typename Sym>
static int docs_launch_ranges(const TokIndexOwner<Sym> &ix, const Sym *dP, const int64_t *dO, int32_t count, uint32_t *dLo, uint32_t *dHi, hipStream_t st)
{
    PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_tok_search, dim3(ngram_grid(count)), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n, dP, dO,
                                                count, (uint8_t *)nullptr, dLo, dHi));
    return SA_AMD_OK;
}

// (a token index keeps no table that belongs to the collection it replaces)
template <typename Sym>
static void docs_replaced(TokIndexOwner<Sym> &) { }

// _set_documents_by_separator behind its argument checks: every occurrence of `sep` ends a document and belongs to it.  The
// separators are counted per tile of the resident text, the counts scanned, and one blocking read-back brings their number k
// and whether a last document runs to n; the offsets table is then allocated at its exact size, written by k_tok_sep_emit, and
// the route is docs_build as for a caller's offsets (its read-back is the sort's error word).  The text is read twice; nothing
// else of its size is touched before docs_build.  A failure leaves the previous collection; *ndocs_out is written last.
template <typename Index>
static int32_t tok_docs_by_separator(Index &ix, uint32_t sep, int64_t *ndocs_out)
{
    const int64_t n = ix.n, tiles = ceil_div(n, TK_TILE);
    PooledScope sc(ix.device, false);
    const size_t wb = docs_layout(ix.n).bytes, b_cnt = align_up((size_t)(tiles + 2) * 8, 256), b_ts = align_up(docs_scan_words(tiles + 1) * 8, 256);
    sc.acquire(wb + b_cnt + b_ts);
    void *dW = sc.take(wb);
    unsigned long long *cnt = (unsigned long long *)sc.take(b_cnt), *tsum = (unsigned long long *)sc.take(b_ts);
    if (sc.rc) return sc.rc;
    hipStream_t st = sc.st;
    const unsigned grid = tok_stream_grid(ceil_div(tiles, TK_SPAN), 1);
    PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_tok_sep_count, dim3(grid), dim3(TK_THREADS), 0, st, ix.text(), n, tiles, sep, cnt));
    { const int rcs = docs_scan(cnt, tiles + 1, tsum, nullptr, st); if (rcs) return rcs; }
    unsigned long long kw[2];
    { const int rcw = read_words(kw, cnt + tiles, sizeof(kw), st); if (rcw) return rcw; }
    if (kw[0] > (unsigned long long)n || kw[1] > 1ull) return SA_AMD_EINTERNAL;
    const int64_t ndocs = (int64_t)(kw[0] + kw[1]);              // (n <= 2^30: far below the byte forms' limit of documents)
    DevBuf off, prev;
    if (index_table_alloc(off, ((size_t)ndocs + 1) * 4) != SA_AMD_OK || index_table_alloc(prev, ((size_t)n + 1) * 4) != SA_AMD_OK) return SA_AMD_ENOMEM;
    PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_tok_sep_emit, dim3(grid), dim3(TK_THREADS), 0, st, ix.text(), n, tiles, sep, (const unsigned long long *)cnt,
                                            off.as<uint32_t>(), kw[0], (uint32_t)kw[1]));
    sc.rc = docs_build(ix.sa(), ix.n, off.as<uint32_t>(), (uint32_t)ndocs, prev.as<uint32_t>(), dW, (int64_t)wb, st);
    if (sc.finish() != SA_AMD_OK) return sc.rc;                  // (a previous collection stays)
    ix.dDocOff = std::move(off);
    ix.dDocPrev = std::move(prev);
    ix.ndocs = (uint32_t)ndocs;
    if (ndocs_out) *ndocs_out = ndocs;
    return SA_AMD_OK;
}

// _doc_offsets: the first min(capacity, ndocs + 1) offsets come down; *ndocs_out behind the copy, which is the step that can fail
template <typename Index>
static int32_t tok_doc_offsets(const Index &ix, uint32_t *doc_off_out, int64_t capacity, int64_t *ndocs_out)
{
    DeviceGuard guard(ix.device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    const int64_t M = (int64_t)ix.ndocs + 1, wr = capacity < M ? capacity : M;
    if (wr > 0) HIP_TRY(hipMemcpy(doc_off_out, ix.doc_off(), (size_t)wr * 4, hipMemcpyDeviceToHost));
    *ndocs_out = (int64_t)ix.ndocs;
    return SA_AMD_OK;
}

template <typename Index>
static int32_t tok_index_sa(const Index &ix, uint32_t *SA_out)
{
    DeviceGuard guard(ix.device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return hipMemcpy(SA_out, ix.sa(), ((size_t)ix.n + 1) * 4, hipMemcpyDeviceToHost) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

// the pattern arguments of the token queries: as search_patterns_valid, offsets in tokens
template <typename Sym>
static bool tok_patterns_valid(const Sym *pat_data, const int64_t *pat_off, int32_t count)
{
    return search_patterns_valid((const uint8_t *)pat_data, pat_off, count);
}

// The host scan of m pattern, prompt or query tokens before anything is uploaded: every id of a 32-bit token text lies below
// 2^24 (any 16-bit value is a token)
template <typename Sym>
static bool tok_ids_valid(const Sym *ids, int64_t m)
{
    if constexpr (sizeof(Sym) == 4)
        for (int64_t i = 0; i < m; ++i)
            if (ids[i] >= TK_LIMIT_U32) return false;
    return true;
}

// what the three query entry points answer before the index is used: SA_AMD_EINVAL for malformed arguments, SA_AMD_ERANGE for a
// pattern id that is no token
template <typename Index>
static int32_t tok_query_args(const Index *ix, const typename Index::Sym *pat_data, const int64_t *pat_off, int32_t count)
{
    if (!ix || !tok_patterns_valid(pat_data, pat_off, count)) return SA_AMD_EINVAL;
    return tok_ids_valid(pat_data, count > 0 ? pat_off[count] : 0) ? SA_AMD_OK : SA_AMD_ERANGE;
}

// _search: host pointers, every output may be nullptr, arguments checked by the caller
template <typename Index>
static int32_t tok_search(const Index &ix, const typename Index::Sym *pat_data, const int64_t *pat_off, int32_t count, uint8_t *contains,
                          uint32_t *range_lo, uint32_t *range_hi)
{
    using Sym = typename Index::Sym;
    if (count == 0) return SA_AMD_OK;
    const size_t C = (size_t)count, total = (size_t)pat_off[count];
    PooledScope sc(ix.device, false);
    const size_t b_pat = align_up(sizeof(Sym) * total + 16, 256), b_off = align_up((C + 1) * 8, 256), b_w = align_up(C * 4 + 4, 256), b_b = align_up(C + 4, 256);
    sc.acquire(b_pat + b_off + 2 * b_w + b_b);
    Sym *dP = (Sym *)sc.take(b_pat);
    int64_t *dO = (int64_t *)sc.take(b_off);
    uint32_t *dLo = (uint32_t *)sc.take(b_w), *dHi = (uint32_t *)sc.take(b_w);
    uint8_t *dC = (uint8_t *)sc.take(b_b);
    if (sc.rc) return sc.rc;
    hipStream_t st = sc.st;
    if (total) HIP_TRY(hipMemcpyAsync(dP, pat_data, sizeof(Sym) * total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dO, pat_off, (C + 1) * 8, hipMemcpyHostToDevice, st));
    PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_tok_search, dim3(ngram_grid(count)), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                (const Sym *)dP, (const int64_t *)dO, count, dC, dLo, dHi));
    if (contains) sc.down(contains, dC, C);
    if (range_lo) sc.down(range_lo, dLo, C * 4);
    if (range_hi) sc.down(range_hi, dHi, C * 4);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    g_prof.resolve();
    return SA_AMD_OK;
}

// backoff == false: _next_tokens (suffix_len is nullptr).  backoff == true: _infgram.  Host
// pointers, every output may be nullptr, arguments checked by the caller.  The steps are those of host/ngram.hpp, in another
// order: the ranges and the counting pass run in one pooled block (8 bytes per query for the listing); a listing has up to
// sym_end<Sym>() entries per query (65 536, or 2^24), so its device side -- min(capacity,
// the counted total) entries -- is a second block taken once the total is known.  One blocking read-back: the total and the
// counters, all of which the counting pass has written.
template <typename Index>
static int tok_query(const Index &ix, const typename Index::Sym *pat_data, const int64_t *pat_off, int32_t count, bool backoff, int32_t min_count,
                     int32_t max_len, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end, int64_t *list_off,
                     typename Index::Sym *tokens, uint32_t *counts, int64_t capacity, int64_t *total_out)
{
    using Sym = typename Index::Sym;
    sa_amd_tok_stats ts = g_last_tok_stats;                     // (the times of the last build stay)
    ngram_stats_fill(ts, ts.compared_tokens, count, backoff, nullptr, 0, 0);
    g_last_tok_stats = ts;
    if (count == 0) {
        if (list_off) list_off[0] = 0;
        if (total_out) *total_out = 0;
        return SA_AMD_OK;
    }
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const int rb0 = g_readbacks;

    PooledScope sc(ix.device, false);
    NgScratch s;
    { const int rcb = ngram_begin(sc, s, pat_data, pat_off, count, sizeof(Sym), 0); if (rcb) return rcb; }
    hipStream_t st = sc.st;

    // ---- the ranges: the plain search, or the back-off ----
    const unsigned grid = ngram_grid(count);
    if (backoff) {
        if constexpr (sizeof(Sym) == 2)
            PROF(KC_MISC, count, st, hipLaunchKernelGGL((k_infgram_suffix<uint16_t>), dim3(grid), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                        (const uint32_t *)nullptr, (const uint64_t *)nullptr, 0, (const uint16_t *)s.pat, (const int64_t *)s.off,
                                                        count, (uint32_t)min_count, (int64_t)max_len, s.len, s.lo, s.hi, s.ctl));
        else
            PROF(KC_MISC, count, st, hipLaunchKernelGGL((k_infgram_suffix<uint32_t>), dim3(grid), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                        (const uint32_t *)nullptr, (const uint64_t *)nullptr, 0, (const uint32_t *)s.pat, (const int64_t *)s.off,
                                                        count, (uint32_t)min_count, (int64_t)max_len, s.len, s.lo, s.hi, s.ctl));
    } else
        PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_tok_search, dim3(grid), dim3(NG_THREADS), 0, st, ix.text(), ix.sa(), (int64_t)ix.n,
                                                    (const Sym *)s.pat, (const int64_t *)s.off, count, (uint8_t *)nullptr, s.lo, s.hi));
    // ---- the continuations: counted, scanned ... ----
    { const int rcn = ngram_count((k_tok_next<false, Sym>), ix.text(), ix.sa(), ix.n, s, backoff, count, st); if (rcn) return rcn; }
    unsigned long long cw[NG_W_COUNT];
    { const int rcw = read_words(cw, s.ctl, sizeof(cw), st); if (rcw) return rcw; }
    const int64_t listed = (int64_t)cw[NG_W_TOTAL];
    if (listed < 0 || listed > (int64_t)sym_end<Sym>() * (int64_t)count) return SA_AMD_EINTERNAL;
    const size_t cap = tokens || counts ? (size_t)(capacity < listed ? capacity : listed) : 0;

    // ---- ... and emitted in order, into a block of the listing's size ----
    PooledScope lsc(-1, false);
    const size_t b_lt = align_up(cap * sizeof(Sym) + 8, 256), b_lc = align_up(cap * 4 + 8, 256);
    Sym *dToks = nullptr;
    uint32_t *dCounts = nullptr;
    if (cap > 0) {
        lsc.acquire(b_lt + b_lc);
        dToks = (Sym *)lsc.take(b_lt);
        dCounts = (uint32_t *)lsc.take(b_lc);
        if (lsc.rc) return lsc.rc;
        const int rce = ngram_pass((k_tok_next<true, Sym>), ix.text(), ix.sa(), ix.n, s, backoff, count, nullptr, tokens ? dToks : nullptr,
                                   counts ? dCounts : nullptr, cap, st);
        if (rce) return rce;
    }

    // ---- down: straight into the caller's arrays ----
    if (tokens && cap > 0) sc.down(tokens, dToks, cap * sizeof(Sym));
    if (counts && cap > 0) sc.down(counts, dCounts, cap * 4);
    ngram_down(sc, s, count, suffix_len, range_lo, range_hi, at_end, list_off);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    if (total_out) *total_out = listed;
    g_prof.resolve();
    ngram_stats_fill(ts, ts.compared_tokens, count, backoff, cw, cap > 0 ? 2 : 1, g_readbacks - rb0);
    g_last_tok_stats = ts;
    return SA_AMD_OK;
}

// ---- the entry points of include/sa_amd_tokdocs.h behind the ABI guard: the argument checks of the byte forms and of
//      tok_query_args, then the shared routes ----

template <typename Index>
static int32_t tokdocs_set(Index *ix, const uint32_t *doc_off, int64_t ndocs)
{
    if (!ix || !docs_valid(doc_off, ndocs) || doc_off[ndocs] != (uint32_t)ix->n) return SA_AMD_EINVAL;
    return docs_set(*ix, doc_off, ndocs);
}

template <typename Index>
static int32_t tokdocs_set_by_separator(Index *ix, uint32_t separator, int64_t *ndocs_out)
{
    if (!ix) return SA_AMD_EINVAL;
    if (separator >= (uint32_t)sym_end<typename Index::Sym>()) return SA_AMD_ERANGE;
    return tok_docs_by_separator(*ix, separator, ndocs_out);
}

template <typename Index>
static int32_t tokdocs_offsets(const Index *ix, uint32_t *doc_off_out, int64_t capacity, int64_t *ndocs_out)
{
    if (!ix || capacity < 0 || !ndocs_out || (capacity > 0 && !doc_off_out) || !ix->doc_off()) return SA_AMD_EINVAL;
    return tok_doc_offsets(*ix, doc_off_out, capacity, ndocs_out);
}

template <typename Index>
static int32_t tokdocs_doc_of(const Index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out)
{
    if (!ix || count < 0 || (count > 0 && (!pos || !doc_out)) || !ix->doc_off()) return SA_AMD_EINVAL;
    if (count == 0) return SA_AMD_OK;
    return doc_of_host(*ix, pos, count, doc_out);
}

// list: the arguments of _doc_list, else those of _doc_search
template <typename Index>
static int32_t tokdocs_query(const Index *ix, const typename Index::Sym *pat_data, const int64_t *pat_off, int32_t count, bool list, uint32_t *occ,
                             uint32_t *df, int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    if (list && (capacity < 0 || !list_off || !total_out || (capacity > 0 && !docs))) return SA_AMD_EINVAL;
    if (const int32_t rc = tok_query_args(ix, pat_data, pat_off, count)) return rc;
    if (!ix->doc_off()) return SA_AMD_EINVAL;
    return docs_query(*ix, pat_data, pat_off, count, list, occ, df, list_off, docs, capacity, total_out);
}

// list: the arguments of _doc_match_list, else those of _doc_match
template <typename Index>
static int32_t tokdocs_match(const Index *ix, const typename Index::Sym *pat_data, const int64_t *pat_off, int32_t npat, const int32_t *clause_off,
                             const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off, int32_t nqueries, bool list, uint32_t *df,
                             uint32_t *clause_df, int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    // (the cast: doc_match_args_valid looks at pat_data for NULL only and at pat_off, which counts symbols of either kind)
    if (!ix || !doc_match_args_valid((const uint8_t *)pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries)) return SA_AMD_EINVAL;
    if (list && (capacity < 0 || !list_off || !total_out || (capacity > 0 && !docs))) return SA_AMD_EINVAL;
    if (!tok_ids_valid(pat_data, npat > 0 ? pat_off[npat] : 0)) return SA_AMD_ERANGE;
    if (!ix->doc_off()) return SA_AMD_EINVAL;
    return doc_match_query(*ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, list, df, clause_df, list_off, docs,
                           capacity, total_out);
}

}  // namespace sa
