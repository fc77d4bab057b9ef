// host/doc_tf.hpp -- per-document term frequencies and top-k documents over a device-resident index (kernels/doc_tf.hpp,
// DESIGN.md section 18): the build of the slots-by-document table behind sa_amd_index_enable_doc_freq, and the two queries
// that run the listing of host/docs.hpp and go on from its device arrays.
#pragma once
#include "docs.hpp"
#include "../kernels/doc_tf.hpp"

namespace sa {

static thread_local sa_amd_doc_tf_stats g_last_doc_tf_stats;
static thread_local int32_t g_topk_piece = -1;          // sa_amd_docs_set_topk_piece of the calling thread (-1: DOC_TOPK_PIECE_DEFAULT)
#ifdef SA_AMD_DIAG
// the second bound of k_doc_tf in the diagnostic library only (sa_amd_debug_doc_tf_bounds): 0 galloping, which is all the product
// library has, 1 a plain binary search -- for the A/B of tools/doc_tf_bench.py and the parity test of tests/test_doc_tf.py
inline std::atomic<int> g_doc_tf_plain_bounds{0};
#endif

// dS (n entries, at least one allocated) from dSA and the resident offsets: the front half of docs_build, then the sorted
// slots themselves.  dWork: docs_layout(n).bytes, 256-byte aligned.  Blocks until done.
static int docs_freq_build(const uint32_t *dSA, int32_t n32, const uint32_t *dOff, uint32_t ndocs, uint32_t *dS, void *dWork, int64_t work_bytes,
                           hipStream_t st)
{
    const int64_t n = n32;
    SortResult<uint32_t> pr;
    uint32_t *ctl = nullptr;
    { const int rcs = docs_sorted_slots(dSA, n32, dOff, ndocs, dWork, work_bytes, st, &pr, &ctl); if (rcs) return rcs; }
    if (n > 0)
        PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_doc_slots, dim3(docs_slot_grid(n)), dim3(DOC_THREADS), 0, st,
                                                (const uint32_t *)(pr.passes ? pr.vals : nullptr), n, dS));
    return docs_built(ctl, st);
}

// sa_amd_index_enable_doc_freq: the table of the index's collection (there is one: checked by the caller); built once
static int32_t docs_freq_enable(sa_amd_index &ix)
{
    if (ix.doc_slots()) return SA_AMD_OK;
    PooledScope sc(ix.device, false);
    if (sc.rc) return sc.rc;
    DevBuf slots;
    if (index_table_alloc(slots, ((size_t)ix.n + 1) * 4) != SA_AMD_OK) return SA_AMD_ENOMEM;      // (n entries; never empty)
    const size_t wb = docs_layout(ix.n).bytes;
    sc.acquire(wb);
    void *dW = sc.take(wb);
    if (sc.rc == SA_AMD_OK) sc.rc = docs_freq_build(ix.sa(), ix.n, ix.doc_off(), ix.ndocs, slots.as<uint32_t>(), dW, (int64_t)wb, sc.st);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    ix.dDocSlots = std::move(slots);
    return SA_AMD_OK;
}

static uint32_t topk_pow2_floor(uint32_t v) { uint32_t p = 1; while (p * 2 <= v) p *= 2; return p; }
static uint32_t topk_pow2_ceil(uint64_t v) { uint32_t p = 1; while (p < v) p *= 2; return p; }

// the effective piece: the thread's switch, raised to at least twice the next power of two >= k (so that k <= P / 2 and a round
// at least halves a list that is longer than P)
static uint32_t topk_piece(int32_t k)
{
    const uint32_t p = (uint32_t)(g_topk_piece < 0 ? DOC_TOPK_PIECE_DEFAULT : g_topk_piece), need = 2 * topk_pow2_ceil((uint64_t)k);
    return p > need ? p : need;
}

// One round of the reduction as the host knows it from the lengths of the lists
struct TopkRound { unsigned long long in_total = 0, pieces = 0, out_total = 0, longest = 0; };

// len (the patterns' list lengths) -> the rounds, the last of which leaves one piece per pattern; len ends as the final lengths
static std::vector<TopkRound> topk_rounds(std::vector<unsigned long long> &len, uint32_t P, uint32_t k)
{
    std::vector<TopkRound> rounds;
    for (;;) {
        TopkRound r;
        bool last = true;
        for (unsigned long long &l : len) {
            const unsigned long long full = l / P, rest = l % P;
            r.in_total += l;
            r.pieces += full + (rest ? 1 : 0);
            if (l > P) last = false;
            const unsigned long long piece = l < P ? l : P;
            if (piece > r.longest) r.longest = piece;
            l = full * k + (rest < k ? rest : k);
            r.out_total += l;
        }
        rounds.push_back(r);
        if (last) return rounds;
    }
}

// k == 0: the listing with a tf next to every document (off_out = list_off, capacity and *total_out as for the listing).
// k >= 1: the top k documents of every pattern (off_out = top_off; docs / tf compact, count * k entries at most).
// Host pointers, docs and tf may be nullptr, arguments checked by the caller.  Read-backs: the listing's (units, list_off),
// the counters of k_doc_tf.
static int doc_tf_query(const sa_amd_index &ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int32_t k, int64_t *off_out,
                        uint32_t *docs, uint32_t *tf, int64_t capacity, int64_t *total_out)
{
    sa_amd_doc_tf_stats ts;
    memset(&ts, 0, sizeof(ts));
    const uint32_t P = k ? topk_piece(k) : 0;
    ts.patterns = count;
    ts.k = k;
    ts.piece = (int32_t)P;
    ts.chunk = (int32_t)(g_docs_chunk < 0 ? DOC_CHUNK_DEFAULT : g_docs_chunk);
    g_last_doc_tf_stats = ts;
    if (count == 0) {
        off_out[0] = 0;
        if (total_out) *total_out = 0;
        return SA_AMD_OK;
    }
    const int rb0 = g_readbacks;
    const size_t C = (size_t)count;
    DocsBatch b(ix.device);
    { const int rcr = docs_ranges(b, ix, pat_data, pat_off, count, true); if (rcr) return rcr; }
    DocsListing ls;
    { const int rcl = docs_listing(b, ls, ix, count, k ? INT64_MAX : capacity); if (rcl) return rcl; }
    if (k && ls.listed > ls.cap) return SA_AMD_EINTERNAL;     // (more than the bound: an array that is no suffix array)
    hipStream_t st = b.sc.st;
    const int64_t entries = ls.listed < ls.cap ? ls.listed : ls.cap;
    ts.occ_sum = (int64_t)b.occ_sum;
    ts.df_sum = ls.listed;

    // ---- the plan of the reduction: the host has list_off, so nothing is read back per round ----
    std::vector<TopkRound> rounds;
    std::vector<unsigned long long> len(k ? C : 0);
    if (k) {
        for (size_t q = 0; q < C; ++q) len[q] = (unsigned long long)(ls.loff[q + 1] - ls.loff[q]);
        rounds = topk_rounds(len, P, (uint32_t)k);
        for (const TopkRound &r : rounds) if (r.pieces > 0x7fffffffull) return SA_AMD_EINTERNAL;
    }
    const unsigned long long top_total = k ? rounds.back().out_total : 0;

    PooledScope s3(-1, false);
    const size_t b_off = align_up((C + 1) * 8, 256), b_ts = align_up(docs_scan_words((int64_t)C + 1) * 8, 256);
    const size_t b_tf = align_up((size_t)entries * 4 + 8, 256), b_keys = align_up((size_t)entries * 8 + 8, 256);
    const size_t b_cand = align_up((size_t)(k && rounds.size() > 1 ? rounds[0].out_total : 0) * 8 + 8, 256);
    const size_t b_top = align_up((size_t)top_total * 4 + 8, 256);
    s3.acquire(k ? b_keys + b_cand + 3 * b_off + b_ts + 2 * b_top : b_tf);
    uint32_t *dTf = nullptr, *dTopDocs = nullptr, *dTopTf = nullptr;
    unsigned long long *keysA = nullptr, *keysB = nullptr, *poff = nullptr, *offA = nullptr, *offB = nullptr, *tsum = nullptr;
    if (k) {
        keysA = (unsigned long long *)s3.take(b_keys); keysB = (unsigned long long *)s3.take(b_cand);
        poff = (unsigned long long *)s3.take(b_off); offA = (unsigned long long *)s3.take(b_off); offB = (unsigned long long *)s3.take(b_off);
        tsum = (unsigned long long *)s3.take(b_ts);
        dTopDocs = (uint32_t *)s3.take(b_top); dTopTf = (uint32_t *)s3.take(b_top);
    } else
        dTf = (uint32_t *)s3.take(b_tf);
    if (s3.rc) return s3.rc;

    // ---- tf of every listed entry (for the top-k: as the reduction's keys) ----
    if (entries > 0) {
        int64_t g = ceil_div(entries, DOC_THREADS);
        const int64_t most = (int64_t)cu_count() * 16;
        if (g > most) g = most;
#ifdef SA_AMD_DIAG
        if (g_doc_tf_plain_bounds.load(std::memory_order_relaxed))
            PROF(KC_MISC, entries, st, hipLaunchKernelGGL((k_doc_tf<false>), dim3((unsigned)g), dim3(DOC_THREADS), 0, st, ix.doc_slots(), ix.doc_off(), ix.ndocs,
                                                          (uint32_t)ix.n, (const uint32_t *)b.dLo, (const uint32_t *)b.dOcc, (const long long *)b.dLoff, count,
                                                          (const uint32_t *)ls.dDocs, entries, dTf, keysA, b.ctl));
        else
#endif
            PROF(KC_MISC, entries, st, hipLaunchKernelGGL((k_doc_tf<true>), dim3((unsigned)g), dim3(DOC_THREADS), 0, st, ix.doc_slots(), ix.doc_off(), ix.ndocs,
                                                          (uint32_t)ix.n, (const uint32_t *)b.dLo, (const uint32_t *)b.dOcc, (const long long *)b.dLoff, count,
                                                          (const uint32_t *)ls.dDocs, entries, dTf, keysA, b.ctl));
    }

    // ---- the rounds: plan, two scans, one workgroup per piece ----
    const unsigned long long *in_off = (const unsigned long long *)b.dLoff, *top_off = nullptr;
    for (size_t r = 0; r < rounds.size(); ++r) {
        const TopkRound &R = rounds[r];
        const bool last = r + 1 == rounds.size();
        unsigned long long *ooff = (r & 1) ? offB : offA;
        const unsigned long long *in = (r & 1) ? keysB : keysA;
        unsigned long long *out = (r & 1) ? keysA : keysB;
        PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_topk_plan, dim3((unsigned)ceil_div((int64_t)count + 1, DOC_THREADS)), dim3(DOC_THREADS), 0, st, in_off,
                                                    count, P, (uint32_t)k, poff, ooff));
        { const int rcn = docs_scan(poff, (int64_t)count + 1, tsum, nullptr, st); if (rcn) return rcn; }
        { const int rcn = docs_scan(ooff, (int64_t)count + 1, tsum, nullptr, st); if (rcn) return rcn; }
        if (R.pieces) {
            uint32_t lds_keys = topk_pow2_ceil(R.longest);
            if (lds_keys < 2) lds_keys = 2;
            PROF(KC_MISC, (int64_t)R.in_total, st, hipLaunchKernelGGL(k_topk_piece, dim3((unsigned)R.pieces), dim3(DOC_TOPK_THREADS), (size_t)lds_keys * 8, st, in,
                                                                      in_off, R.in_total, (const unsigned long long *)poff, (const unsigned long long *)ooff,
                                                                      count, P, (uint32_t)k, lds_keys, last ? (unsigned long long *)nullptr : out,
                                                                      last ? dTopDocs : (uint32_t *)nullptr, last ? dTopTf : (uint32_t *)nullptr, R.out_total));
        }
        ts.pieces += (int64_t)R.pieces;
        in_off = top_off = ooff;
    }
    ts.rounds = (int32_t)rounds.size();

    unsigned long long cw[5] = {0, 0, 0, 0, 0};
    { const int rcw = read_words(cw, b.ctl, sizeof(cw), st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    ts.table_loads = (int64_t)cw[3];
    ts.tf_sum = (int64_t)cw[4];

    // ---- down: the two downloads are the last steps that can fail (each straight into the caller's array: a staging copy of
    // the listing's 4 df_sum bytes on the host cost more than all the kernels); the offsets and the total go behind them ----
    const int64_t wr = k ? (int64_t)top_total : entries;
    std::vector<int64_t> toff(k ? C + 1 : 0);
    if (k) b.sc.down(toff.data(), top_off, (C + 1) * 8);
    if (b.sc.rc) return b.sc.rc;
    if (k && toff[C] != (int64_t)top_total) return SA_AMD_EINTERNAL;
    if (s3.finish() != SA_AMD_OK) return s3.rc;
    if (ls.s2.finish() != SA_AMD_OK) return ls.s2.rc;
    if (b.sc.finish() != SA_AMD_OK) return b.sc.rc;
    if (tf && wr > 0) HIP_TRY(hipMemcpy(tf, k ? dTopTf : dTf, (size_t)wr * 4, hipMemcpyDeviceToHost));
    if (docs && wr > 0) HIP_TRY(hipMemcpy(docs, k ? dTopDocs : ls.dDocs, (size_t)wr * 4, hipMemcpyDeviceToHost));
    memcpy(off_out, k ? toff.data() : ls.loff.data(), (C + 1) * 8);
    if (total_out) *total_out = ls.listed;
    ts.topk_entries = (int64_t)top_total;
    g_prof.resolve();
    ts.readbacks = g_readbacks - rb0;
    g_last_doc_tf_stats = ts;
    return SA_AMD_OK;
}

}  // namespace sa
