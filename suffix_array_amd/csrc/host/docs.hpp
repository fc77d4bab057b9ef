// host/docs.hpp -- document collections over a device-resident index (kernels/docs.hpp): the build of
// the per-slot word behind sa_amd_index_set_documents, positions to documents, document frequency and document listing.
#pragma once
#include "scope.hpp"
#include "esa.hpp"
#include "index.hpp"
#include "../kernels/docs.hpp"

namespace sa {

static thread_local sa_amd_docs_stats g_last_docs_stats;
static thread_local int32_t g_docs_chunk = -1;          // sa_amd_docs_set_chunk of the calling thread (-1: DOC_CHUNK_DEFAULT)

// layout of the build's work block: control words (the sort's error word first) | four (n + 1)-entry buffers (the document ids
// of the slots, the sort's values and their two alternates) | sort spine | single-pass granules.  About 16 bytes per byte of text.
struct DocsLayout { size_t ctl, keys, vals, altk, altv, alt_elems, spine, status, bytes; };
static DocsLayout docs_layout(int32_t n)
{
    DocsLayout L;
    const size_t N1 = (size_t)n + 1;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = align_up(off + b, 256); return o; };
    L.ctl = take(256);
    L.alt_elems = (N1 + 67) & ~(size_t)3;
    L.keys = take(L.alt_elems * 4);
    L.vals = take(L.alt_elems * 4);
    L.altk = take(L.alt_elems * 4);
    L.altv = take(L.alt_elems * 4);
    L.spine = take(SortScratch::SPINE_BYTES);
    L.status = take(SortScratch::granule_bytes((int64_t)N1));
    L.bytes = off;
    return L;
}

// doc_off[0 .. ndocs]: starts at 0 and never decreases (the caller compares the last entry with the index's n)
static bool docs_valid(const uint32_t *doc_off, int64_t ndocs)
{
    if (!doc_off || ndocs < 1 || ndocs > (int64_t)0xfffffffe) return false;
    if (doc_off[0] != 0) return false;
    for (int64_t d = 0; d < ndocs; ++d) if (doc_off[d + 1] < doc_off[d]) return false;
    return true;
}

static int launch_doc_of(const uint32_t *dPos, int64_t count, const uint32_t *dOff, uint32_t ndocs, int32_t n, uint32_t *dOut, hipStream_t st)
{
    if (count <= 0) return SA_AMD_OK;
    const uint32_t M = ndocs + 1;
    const uint32_t stride = (uint32_t)ceil_div((int64_t)M, DOC_SAMPLES), ns = (uint32_t)ceil_div((int64_t)M, stride);
    int64_t g = ceil_div(count, (int64_t)DOC_THREADS * DOC_ITEMS);
    const int64_t most = (int64_t)cu_count() * 8;
    if (g > most) g = most;
    PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_doc_of, dim3((unsigned)g), dim3(DOC_THREADS), 0, st, dPos, count, dOff, M, stride, ns, (uint32_t)n, dOut));
    return SA_AMD_OK;
}

// The front half of every table build: DA of slots 1 .. n (slot 0 is the empty suffix: no document), then the slots in stable
// order of their document.  pr->keys: the document ids in that order, pr->vals: the slots less one (only when pr->passes: one
// document sorts nothing and the order is that of the slots).  dWork: docs_layout(n).bytes, 256-byte aligned; *ctl_out: its
// control words, the sort's error word first.
static int docs_sorted_slots(const uint32_t *dSA, int32_t n32, const uint32_t *dOff, uint32_t ndocs, void *dWork, int64_t work_bytes, hipStream_t st,
                             SortResult<uint32_t> *pr, uint32_t **ctl_out)
{
    const int64_t n = n32;
    const DocsLayout L = docs_layout(n32);
    if (!dWork || work_bytes < (int64_t)L.bytes || (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;
    const Tuning tn = route_tuning();
    char *base = (char *)dWork;
    uint32_t *ctl = (uint32_t *)(base + L.ctl);
    uint32_t *keys = (uint32_t *)(base + L.keys), *vals = (uint32_t *)(base + L.vals);
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    const SortScratch ss = SortScratch::make(base + L.spine, base + L.status, ctl);
    { const int rcd = launch_doc_of(dSA + 1, n, dOff, ndocs, n32, keys, st); if (rcd) return rcd; }
    *ctl_out = ctl;
    SortJob<uint32_t> job{ keys, vals, (uint32_t *)(base + L.altk), (uint32_t *)(base + L.altv), n, 0, bit_length((uint64_t)ndocs - 1) };
    job.iota = true;
    return sort_pairs32(job, ss, st, tn, pr);
}

// the end of every table build: the sort's error word comes back; blocks until the table is written
static int docs_built(const uint32_t *ctl, hipStream_t st)
{
    uint32_t err = 0;
    { const int rcw = read_words(&err, ctl, 4, st); if (rcw) return rcw; }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    if (err) return SA_AMD_EINTERNAL;               // a look-back of the sort gave up (never seen; never a silent wrong table)
    return SA_AMD_OK;
}

static unsigned docs_slot_grid(int64_t n)
{
    int64_t g = ceil_div(n, DOC_THREADS);
    if (g > 16384) g = 16384;
    return (unsigned)(g < 1 ? 1 : g);
}

// dPrev (n + 1 entries) from dSA and the uploaded offsets; dWork: docs_layout(n).bytes, 256-byte aligned.  Blocks until done.
static int docs_build(const uint32_t *dSA, int32_t n32, const uint32_t *dOff, uint32_t ndocs, uint32_t *dPrev, void *dWork, int64_t work_bytes,
                      hipStream_t st)
{
    const int64_t n = n32;
    SortResult<uint32_t> pr;
    uint32_t *ctl = nullptr;
    { const int rcs = docs_sorted_slots(dSA, n32, dOff, ndocs, dWork, work_bytes, st, &pr, &ctl); if (rcs) return rcs; }
    PROF(KC_MISC, n, st, hipLaunchKernelGGL(k_doc_prev, dim3(docs_slot_grid(n)), dim3(DOC_THREADS), 0, st, (const uint32_t *)pr.keys,
                                            (const uint32_t *)(pr.passes ? pr.vals : nullptr), n, dPrev));
    return docs_built(ctl, st);
}

// exclusive scan of v[0 .. len) in place; tsum: ceil(len / DOC_SCAN_TILE) words; last_out: see k_doc_scan_tiles
static int docs_scan(unsigned long long *v, int64_t len, unsigned long long *tsum, unsigned long long *last_out, hipStream_t st)
{
    const int64_t tiles = ceil_div(len, DOC_SCAN_TILE);
    PROF(KC_MISC, len, st, hipLaunchKernelGGL((k_doc_scan_tiles<0>), dim3((unsigned)tiles), dim3(DOC_SCAN_THREADS), 0, st, v, len, tsum,
                                              (unsigned long long *)nullptr));
    PROF(KC_MISC, tiles, st, hipLaunchKernelGGL(k_doc_scan_spine, dim3(1), dim3(DOC_SPINE_THREADS), 0, st, tsum, tiles));
    PROF(KC_MISC, len, st, hipLaunchKernelGGL((k_doc_scan_tiles<1>), dim3((unsigned)tiles), dim3(DOC_SCAN_THREADS), 0, st, v, len, tsum, last_out));
    return SA_AMD_OK;
}

static size_t docs_scan_words(int64_t len) { return (size_t)ceil_div(len, DOC_SCAN_TILE) + 1; }

static unsigned docs_unit_grid(int64_t units)
{
    int64_t g = ceil_div(units, DOC_THREADS / WAVE);
    const int64_t most = (int64_t)cu_count() * 16;
    if (g > most) g = most;
    return (unsigned)(g < 1 ? 1 : g);
}

// The device side of a batch of patterns after its ranges: lo (clamped), occ, the scanned units and their totals.  With `list`
// the block has room for the listing's offsets as well.
struct DocsBatch {
    PooledScope sc;
    unsigned long long *ctl = nullptr, *uoff = nullptr;
    uint32_t *dLo = nullptr, *dOcc = nullptr, *dDf = nullptr;
    long long *dLoff = nullptr;
    uint32_t chunk = 0;
    unsigned long long units = 0, occ_sum = 0, bound = 0;
    explicit DocsBatch(int device) : sc(device, false) {}
};

// What an index type supplies to the document routes below, which are written once over it: the symbol
// of its patterns, DocsSym<Index>::type, and the range step, docs_launch_ranges(ix, dP, dO, count, dLo, dHi, st) -- an
// overload found through the index type.  Everything else they use is common to the owners: device, n, ndocs, sa(), doc_off(),
// doc_prev().  The byte index: bytes, and the search kernels with the bucket and LCP tables as sa_amd_index_search runs them.
template <typename Index> struct DocsSym { using type = typename Index::Sym; };
template <> struct DocsSym<sa_amd_index> { using type = uint8_t; };

static int docs_launch_ranges(const sa_amd_index &ix, const uint8_t *dP, const int64_t *dO, int32_t count, uint32_t *dLo, uint32_t *dHi, hipStream_t st)
{
    g_prof.begin(KC_MISC, count, st);
    const int rcs = launch_search(ix.text(), ix.sa(), ix.n, ix.bkt(), ix.pair(), dP, dO, count, nullptr, dLo, dHi, nullptr, nullptr, nullptr, st);
    g_prof.end(st);
    return rcs;
}

// the end of docs_set: the tables a replaced collection leaves behind.  The byte index drops the frequency table, which was the
// old collection's.
static void docs_replaced(sa_amd_index &ix) { ix.dDocSlots.reset(); }

// patterns up, the ranges by the index's range step, the units.  One blocking read-back: the number of units (with the summed
// occ and the bound of the listing).  count >= 1; pat_off counts symbols.
template <typename Index>
static int docs_ranges(DocsBatch &b, const Index &ix, const typename DocsSym<Index>::type *pat_data, const int64_t *pat_off, int32_t count, bool list)
{
    using Sym = typename DocsSym<Index>::type;
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const size_t C = (size_t)count, total = sizeof(Sym) * (size_t)pat_off[count];
    const uint32_t N1 = (uint32_t)ix.n + 1u;
    b.chunk = (uint32_t)(g_docs_chunk < 0 ? DOC_CHUNK_DEFAULT : g_docs_chunk);
    const uint32_t chunk = b.chunk;

    PooledScope &sc = b.sc;
    const size_t b_pat = align_up(total + 16, 256), b_off = align_up((C + 1) * 8, 256), b_w = align_up(C * 4 + 4, 256);
    const size_t b_ts = align_up(docs_scan_words((int64_t)C + 1) * 8, 256);
    sc.acquire(256 + b_pat + b_off + 4 * b_w + b_off + b_ts + (list ? b_off : 0));
    unsigned long long *ctl = b.ctl = (unsigned long long *)sc.take(256);
    Sym *dP = (Sym *)sc.take(b_pat);
    int64_t *dO = (int64_t *)sc.take(b_off);
    uint32_t *dLo = b.dLo = (uint32_t *)sc.take(b_w), *dHi = (uint32_t *)sc.take(b_w);
    b.dOcc = (uint32_t *)sc.take(b_w);
    b.dDf = (uint32_t *)sc.take(b_w);
    unsigned long long *uoff = b.uoff = (unsigned long long *)sc.take(b_off), *tsum = (unsigned long long *)sc.take(b_ts);
    b.dLoff = list ? (long long *)sc.take(b_off) : nullptr;
    if (sc.rc) return sc.rc;
    hipStream_t st = sc.st;
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    HIP_TRY(hipMemsetAsync(b.dDf, 0, C * 4, st));
    if (total) HIP_TRY(hipMemcpyAsync(dP, pat_data, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dO, pat_off, (C + 1) * 8, hipMemcpyHostToDevice, st));

    // ---- the ranges, as the index's own search runs them ----
    { const int rcs = docs_launch_ranges(ix, (const Sym *)dP, (const int64_t *)dO, count, dLo, dHi, st); if (rcs) return rcs; }
    // ---- the units: ceil(occ / chunk) per pattern, scanned; the number of all of them comes back ----
    PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_doc_ranges, dim3((unsigned)ceil_div((int64_t)count + 1, DOC_THREADS)), dim3(DOC_THREADS), 0, st, dLo,
                                                (const uint32_t *)dHi, count, N1, chunk, ix.ndocs, b.dOcc, uoff, ctl));
    { const int rcn = docs_scan(uoff, (int64_t)count + 1, tsum, &ctl[0], st); if (rcn) return rcn; }
    unsigned long long cw[3];
    { const int rcw = read_words(cw, ctl, sizeof(cw), st); if (rcw) return rcw; }
    b.units = cw[0]; b.occ_sum = cw[1]; b.bound = cw[2];
    if (b.units > (unsigned long long)count + b.occ_sum / chunk || b.occ_sum > (unsigned long long)count * N1) return SA_AMD_EINTERNAL;
    return SA_AMD_OK;
}

// The listing of a batch on the device: the first `cap` = min(capacity, bound) documents in dDocs, the offsets of all of them in
// loff (count + 1 entries, on the host), their number in `listed`.  Its scratch is a block of its own, sized by the units.
struct DocsListing {
    PooledScope s2;
    uint32_t *dDocs = nullptr;
    int64_t cap = 0, listed = 0;
    std::vector<int64_t> loff;
    DocsListing() : s2(-1, false) {}
};

// counts per unit, one scan for the units' offsets and the patterns', ordered compaction; waits for the stream
template <typename Index>
static int docs_listing(DocsBatch &b, DocsListing &ls, const Index &ix, int32_t count, int64_t capacity)
{
    const size_t C = (size_t)count;
    const unsigned long long units = b.units, occ_sum = b.occ_sum;
    const uint32_t chunk = b.chunk;
    hipStream_t st = b.sc.st;
    const int64_t cap = ls.cap = capacity < (int64_t)b.bound ? capacity : (int64_t)b.bound;
    const size_t b_uc = align_up(((size_t)units + 1) * 8, 256), b_uq = align_up((size_t)units * 4 + 4, 256);
    const size_t b_ut = align_up(docs_scan_words((int64_t)units + 1) * 8, 256), b_docs = align_up((size_t)cap * 4 + 8, 256);
    PooledScope &s2 = ls.s2;
    s2.acquire(b_uc + b_uq + b_ut + b_docs);
    unsigned long long *ucnt = (unsigned long long *)s2.take(b_uc), *utsum = (unsigned long long *)s2.take(b_ut);
    uint32_t *uq = (uint32_t *)s2.take(b_uq), *dDocs = ls.dDocs = (uint32_t *)s2.take(b_docs);
    if (s2.rc) return s2.rc;
    HIP_TRY(hipMemsetAsync(ucnt + units, 0, 8, st));
    if (units)
        PROF(KC_MISC, (int64_t)occ_sum, st, hipLaunchKernelGGL((k_doc_count<true>), dim3(docs_unit_grid((int64_t)units)), dim3(DOC_THREADS), 0, st, ix.doc_prev(),
                                                               (const uint32_t *)b.dLo, (const uint32_t *)b.dOcc, (const unsigned long long *)b.uoff, count, units,
                                                               chunk, (uint32_t *)nullptr, ucnt, uq));
    { const int rcn = docs_scan(ucnt, (int64_t)units + 1, utsum, nullptr, st); if (rcn) return rcn; }
    PROF(KC_MISC, count, st, hipLaunchKernelGGL(k_doc_list_off, dim3((unsigned)ceil_div((int64_t)count + 1, DOC_THREADS)), dim3(DOC_THREADS), 0, st,
                                                (const unsigned long long *)b.uoff, (const unsigned long long *)ucnt, units, count, b.dLoff));
    if (units && cap > 0)
        PROF(KC_MISC, (int64_t)occ_sum, st, hipLaunchKernelGGL(k_doc_emit, dim3(docs_unit_grid((int64_t)units)), dim3(DOC_THREADS), 0, st, ix.doc_prev(), ix.sa(),
                                                               (const uint32_t *)b.dLo, (const uint32_t *)b.dOcc, (const unsigned long long *)b.uoff,
                                                               (const uint32_t *)uq, (const unsigned long long *)ucnt, units, count, chunk, ix.doc_off(),
                                                               ix.ndocs + 1u, (uint32_t)ix.n, dDocs, (unsigned long long)cap));
    HIP_TRY(hipStreamSynchronize(st));
    ls.loff.resize(C + 1);
    b.sc.down(ls.loff.data(), b.dLoff, (C + 1) * 8);
    if (b.sc.rc) return b.sc.rc;
    ls.listed = ls.loff[C];
    if (ls.listed < 0) return SA_AMD_EINTERNAL;               // (above `bound` only for an array that is no suffix array: what fits `cap` is written)
    return SA_AMD_OK;
}

// Document frequency (!list: occ and df, either may be nullptr) or listing (list_off: count + 1 entries, the first `capacity`
// documents to docs, the number of all of them to *total_out) of a batch of patterns; host pointers, arguments checked by the
// caller.
template <typename Index>
static int docs_query(const Index &ix, const typename DocsSym<Index>::type *pat_data, const int64_t *pat_off, int32_t count, bool list, uint32_t *occ_out,
                      uint32_t *df_out, int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    sa_amd_docs_stats ds;
    memset(&ds, 0, sizeof(ds));
    ds.patterns = count;
    ds.chunk = (int32_t)(g_docs_chunk < 0 ? DOC_CHUNK_DEFAULT : g_docs_chunk);
    ds.listed = list ? 1 : 0;
    g_last_docs_stats = ds;
    if (count == 0) {
        if (list) { list_off[0] = 0; *total_out = 0; }
        return SA_AMD_OK;
    }
    const int rb0 = g_readbacks;
    const size_t C = (size_t)count;
    DocsBatch b(ix.device);
    { const int rcr = docs_ranges(b, ix, pat_data, pat_off, count, list); if (rcr) return rcr; }
    PooledScope &sc = b.sc;
    hipStream_t st = sc.st;
    ds.occ_sum = (int64_t)b.occ_sum;
    ds.units = (int64_t)b.units;
    ds.slots_scanned = (int64_t)b.occ_sum * (list ? 2 : 1);

    if (!list) {
        std::vector<uint32_t> df(C);
        if (b.units)
            PROF(KC_MISC, (int64_t)b.occ_sum, st, hipLaunchKernelGGL((k_doc_count<false>), dim3(docs_unit_grid((int64_t)b.units)), dim3(DOC_THREADS), 0, st,
                                                                     ix.doc_prev(), (const uint32_t *)b.dLo, (const uint32_t *)b.dOcc,
                                                                     (const unsigned long long *)b.uoff, count, b.units, b.chunk, b.dDf,
                                                                     (unsigned long long *)nullptr, (uint32_t *)nullptr));
        HIP_TRY(hipStreamSynchronize(st));
        sc.down(df.data(), b.dDf, C * 4);
        if (sc.finish() != SA_AMD_OK) return sc.rc;
        if (occ_out) HIP_TRY(hipMemcpy(occ_out, b.dOcc, C * 4, hipMemcpyDeviceToHost));      // the last step that can fail: nothing else is written before it
        for (size_t q = 0; q < C; ++q) ds.df_sum += df[q];
        if (df_out) memcpy(df_out, df.data(), C * 4);
    } else {
        DocsListing ls;
        { const int rcl = docs_listing(b, ls, ix, count, capacity); if (rcl) return rcl; }
        const int64_t wr = ls.listed < ls.cap ? ls.listed : ls.cap;
        if (ls.s2.finish() != SA_AMD_OK) return ls.s2.rc;
        if (sc.finish() != SA_AMD_OK) return sc.rc;
        if (wr > 0) HIP_TRY(hipMemcpy(docs, ls.dDocs, (size_t)wr * 4, hipMemcpyDeviceToHost));    // the last step that can fail; list_off and the total behind it
        memcpy(list_off, ls.loff.data(), (C + 1) * 8);
        *total_out = ls.listed;
        ds.df_sum = ls.listed;
    }
    g_prof.resolve();
    ds.readbacks = g_readbacks - rb0;
    g_last_docs_stats = ds;
    return SA_AMD_OK;
}

// sa_amd_index_set_documents and the token indexes' _set_documents: the collection's two tables, built from the caller's offsets
// (checked by the caller) and handed to the index.  A failure leaves the previous collection and (the byte index) its frequency
// table; a success drops that table, which was the old collection's: the caller enables it again.
template <typename Index>
static int32_t docs_set(Index &ix, const uint32_t *doc_off, int64_t ndocs)
{
    const size_t M = (size_t)ndocs + 1, N1 = (size_t)ix.n + 1;
    PooledScope sc(ix.device, false);
    if (sc.rc) return sc.rc;
    DevBuf off, prev;
    if (index_table_alloc(off, M * 4) != SA_AMD_OK || index_table_alloc(prev, N1 * 4) != SA_AMD_OK) return SA_AMD_ENOMEM;
    const size_t wb = docs_layout(ix.n).bytes;
    sc.acquire(wb);
    void *dW = sc.take(wb);
    if (sc.rc == SA_AMD_OK) sc.rc = hip_status(hipMemcpy(off.p, doc_off, M * 4, hipMemcpyHostToDevice));
    if (sc.rc == SA_AMD_OK) sc.rc = docs_build(ix.sa(), ix.n, off.as<uint32_t>(), (uint32_t)ndocs, prev.as<uint32_t>(), dW, (int64_t)wb, sc.st);
    if (sc.finish() != SA_AMD_OK) return sc.rc;                  // (a previous collection stays)
    ix.dDocOff = std::move(off);
    ix.dDocPrev = std::move(prev);
    docs_replaced(ix);
    ix.ndocs = (uint32_t)ndocs;
    return SA_AMD_OK;
}

// sa_amd_index_doc_of and the token indexes' _doc_of: host pointers, count >= 1
template <typename Index>
static int32_t doc_of_host(const Index &ix, const uint32_t *pos, int64_t count, uint32_t *doc_out)
{
    const size_t b = align_up((size_t)count * 4, 256);
    PooledScope sc(ix.device, false);
    sc.acquire(2 * b);
    uint32_t *dPos = (uint32_t *)sc.take(b), *dOut = (uint32_t *)sc.take(b);
    if (sc.rc == SA_AMD_OK) sc.rc = hip_status(hipMemcpyAsync(dPos, pos, (size_t)count * 4, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK) sc.rc = launch_doc_of(dPos, count, ix.doc_off(), ix.ndocs, ix.n, dOut, sc.st);
    sc.down(doc_out, dOut, (size_t)count * 4);
    return sc.finish();
}

// sa_amd_index_doc_of_device: pointers on the index's device, count >= 1.  Blocks until done.
static int32_t doc_of_device(const sa_amd_index &ix, const uint32_t *dPos, int64_t count, uint32_t *dDoc, hipStream_t st)
{
    DeviceGuard guard(ix.device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    const int32_t rc = launch_doc_of(dPos, count, ix.doc_off(), ix.ndocs, ix.n, dDoc, st);
    if (rc) return rc;
    return hip_status(hipStreamSynchronize(st));
}

}  // namespace sa
