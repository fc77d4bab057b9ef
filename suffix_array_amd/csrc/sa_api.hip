// sa_api.hip -- the C ABI (include/suffix_array_amd.h) of the MI355X-native suffix-array construction engine.
// Replaces the body of `saca()` (reference src/saca.rs:9-15) and the C engine behind
// `cdivsufsort::sort_in_place` (src/saca.rs:14).
//
// There is deliberately no CPU fallback: every entry point runs the HIP kernels of kernels/*.hpp or returns an
// error code.  Nothing unwinds through the ABI (SA_ABI_GUARD_*), device buffers are RAII (DevBuf), and an entry point
// that switches the HIP device restores the caller's device before it returns (DeviceGuard).
//
// One translation unit, two products (csrc/Makefile):
//   libsuffix_array_amd.so        this file as is: bit-exact under ANY environment
//   libsuffix_array_amd_diag.so   -DSA_AMD_DIAG: adds the timing ablations (wrong orders on purpose), phase stamps and
//                                 the primitive test hooks of sa_diag.inc -- used by tools/ and the primitive tests only
#include "host/support.hpp"
#include "host/tuning.hpp"
#include "host/pipeline.hpp"
#include "host/host_path.hpp"
#include "host/lcp.hpp"
#include "host/esa.hpp"
#include "host/bwt.hpp"
#include "host/repeats.hpp"
#include "host/lz.hpp"
#include "host/match.hpp"
#include "host/docs.hpp"
#include "host/doc_repeats.hpp"
#include "host/doc_tf.hpp"

extern "C" {

#define SA_EXPORT __attribute__((visibility("default")))

SA_EXPORT int32_t sa_amd_max_length(void) { return SA_AMD_MAX_LENGTH; }

SA_EXPORT int32_t sa_amd_divsufsort(const uint8_t *T, int32_t *SA, int32_t n)
{
    SA_ABI_GUARD_BEGIN
    return sa::build_host(T, (uint32_t *)SA, n, false, sa::pick_device());
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_saca_u8(const uint8_t *T, uint32_t *SA, int32_t n)
{
    SA_ABI_GUARD_BEGIN
    return sa::build_host(T, SA, n, true, sa::pick_device());
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_saca_batch(const uint8_t *const *T, uint32_t *const *SA, const int32_t *n, const int32_t *device,
                                    int32_t count, int32_t *status)
{
    if (count < 0 || (count > 0 && (!T || !SA || !n))) return SA_AMD_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    std::vector<int32_t> st((size_t)count, SA_AMD_OK);
    std::vector<std::vector<int>> per_dev((size_t)ndev), small_dev((size_t)ndev);
    // texts of up to SA_AMD_SMALL_MAX bytes (the one-workgroup kernel's) are built together, one launch per device and chunk
    // (host/host_path.hpp, build_host_small_batch) -- unless a device has a single one, which takes the single-call path
    const sa::HostTuning ht = sa::HostTuning::from_env();
    for (int i = 0; i < count; ++i) {
        const int d = device ? device[i] : i % ndev;
        if (d < 0 || d >= ndev) { st[(size_t)i] = SA_AMD_EINVAL; continue; }
        if (n[i] > 0 && n[i] <= ht.small_max && T[i] && SA[i]) small_dev[(size_t)d].push_back(i);
        else per_dev[(size_t)d].push_back(i);
    }
    for (int d = 0; d < ndev; ++d)
        if (small_dev[(size_t)d].size() == 1) { per_dev[(size_t)d].push_back(small_dev[(size_t)d][0]); small_dev[(size_t)d].clear(); }
    std::vector<std::atomic<int>> small_taken((size_t)ndev);
    for (auto &a : small_taken) a.store(0);
    // Two host threads per device (SA_AMD_BATCH_THREADS, 1..16), each with its own stream and device block, take the
    // device's items in turn: while one waits for its 4(n+1)-byte copy back over PCIe the other uploads and computes,
    // so the link and the GPU overlap instead of alternating.
    // (SA_AMD_BATCH_THREADS = 0, the default: two per device; six for a device whose texts are all below SA_AMD_LANES_MIN_N, twelve
    // when they are all below 8 MiB -- those builds leave most of the GPU idle and take no turns, host/host_path.hpp; measured,
    // one GPU: 128 x 1 MiB of English 196 ms with two threads and turns, 67 with eight, 58 with twelve; 16 x 16 MiB 75 / 65 / 71)
    const int per_env = (int)sa::env_int("SA_AMD_BATCH_THREADS", 0, 0, 16);
    const int64_t lanes_min = ht.lanes_min_n;
    std::vector<int> per_of((size_t)ndev, 2);
    for (int d = 0; d < ndev; ++d) {
        int64_t largest = 0;
        for (int i : per_dev[(size_t)d]) largest = n[i] > largest ? n[i] : largest;
        per_of[(size_t)d] = per_env > 0 ? per_env : (largest < lanes_min ? (largest < ((int64_t)8 << 20) ? 12 : 6) : 2);
    }
    std::vector<std::atomic<size_t>> next((size_t)ndev);
    for (auto &a : next) a.store(0);
    auto work = [&](int d) {
        if (!small_dev[(size_t)d].empty() && small_taken[(size_t)d].exchange(1) == 0) {
            // (the first worker of the device to get here; the others go on with the large texts meanwhile)
            try { (void)sa::build_host_small_batch(T, SA, n, small_dev[(size_t)d].data(), small_dev[(size_t)d].size(), d, st.data()); }
            catch (const std::bad_alloc &) { for (int i : small_dev[(size_t)d]) st[(size_t)i] = SA_AMD_ENOMEM; }
            catch (...) { for (int i : small_dev[(size_t)d]) st[(size_t)i] = SA_AMD_EINTERNAL; }
        }
        for (;;) {
            const size_t q = next[(size_t)d].fetch_add(1);
            if (q >= per_dev[(size_t)d].size()) break;
            const int i = per_dev[(size_t)d][q];
            int32_t rc;
            try { rc = sa::build_host(T[i], SA[i], n[i], true, d); }
            catch (const std::bad_alloc &) { rc = SA_AMD_ENOMEM; }
            catch (...) { rc = SA_AMD_EINTERNAL; }
            st[(size_t)i] = rc;
        }
    };
    std::vector<std::thread> workers;
    bool spawn_failed = false;
    for (int d = 0; d < ndev && !spawn_failed; ++d) {
        const size_t items = per_dev[(size_t)d].size() + (small_dev[(size_t)d].empty() ? 0 : 1);
        for (int k = 0; k < per_of[(size_t)d] && (size_t)k < items; ++k) {
            try { workers.emplace_back(work, d); }
            catch (...) { spawn_failed = true; break; }         // (std::system_error: no more threads)
        }
    }
    for (auto &t : workers) t.join();
    if (spawn_failed)
        for (int d = 0; d < ndev; ++d) work(d);                  // whatever the started workers left is done here, serially
    int32_t first = SA_AMD_OK;
    for (int i = 0; i < count; ++i) {
        if (status) status[i] = st[(size_t)i];
        if (first == SA_AMD_OK && st[(size_t)i] != SA_AMD_OK) first = st[(size_t)i];
    }
    return first;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int64_t sa_amd_workspace_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::carve(nullptr, n).bytes;
}

SA_EXPORT int32_t sa_amd_saca_device(const uint8_t *dT, uint32_t *dSA, int32_t n, void *dWork, int64_t work_bytes,
                                     void *stream, sa_amd_stats *stats)
{
    if (n < 0 || !dSA || (n > 0 && (!dT || !dWork))) return SA_AMD_EINVAL;
    if (n > 0 && (((uintptr_t)dWork) & 255u)) return SA_AMD_EINVAL;       // the carved slabs are read with 16-byte vector loads
    SA_ABI_GUARD_BEGIN
    return sa::build_device(dT, dSA, n, dWork, work_bytes, (hipStream_t)stream, stats);
    SA_ABI_GUARD_END(0)
}

// ---- next rows: bucket table and integrity check on the device-resident arrays ----

SA_EXPORT int32_t sa_amd_bucket_table_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dBkt, void *stream)
{
    SA_ABI_GUARD_BEGIN
    if (n < 0 || !dBkt || (n > 0 && !dT)) return SA_AMD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (dSA) {
        // a device-resident index has the sorted order at hand: one binary search per bucket edge (~0.08 ms whatever n)
        hipLaunchKernelGGL(sa::k_bucket_table, dim3((sa::BKT_LEN + 255) / 256), dim3(256), 0, st, dT, dSA, (int64_t)n, dBkt);
    } else {
        // as the reference builds it (src/sa.rs:96-116): bigram counts of the text + prefix sum, no suffix array needed.  The
        // counts live in the first 65 536 words of dBkt itself (k_bigram_scan reads them all before it writes)
        if (hipMemsetAsync(dBkt, 0, (size_t)65536 * 4, st) != hipSuccess) return SA_AMD_EHIP;
        int64_t pairs = sa::ceil_div((int64_t)n, sa::BG_MIN_CHUNK);
        if (pairs > sa::BG_MAX_PAIRS) pairs = sa::BG_MAX_PAIRS;
        if (n >= 2)
            hipLaunchKernelGGL(sa::k_bigram_hist, dim3((unsigned)(2 * pairs)), dim3(sa::BG_THREADS), 0, st, dT, (int64_t)n, (int)pairs, dBkt);
        hipLaunchKernelGGL(sa::k_bigram_scan, dim3(1), dim3(sa::BGS_THREADS), 0, st, (const uint32_t *)dBkt, dT, (int64_t)n, dBkt);
    }
    if (hipGetLastError() != hipSuccess) return SA_AMD_EHIP;
    return hipStreamSynchronize(st) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
    SA_ABI_GUARD_END(0)
}

// layout of the larger work block (fast form): flags | rank | four pair buffers | spine + digit totals | granules + error word
struct CiLayout { size_t flags, rank, alt, alt_elems, spine, status, err, starts, bitmap, bitmap_bytes, bytes; };
static CiLayout ci_layout(int32_t n)
{
    CiLayout L;
    const size_t N1 = (size_t)n + 1;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = sa::align_up(off + b, 256); return o; };
    L.flags = take(256);
    L.rank = take(N1 * 4);
    L.alt_elems = (N1 + 67) & ~(size_t)3;
    L.alt = take(4 * L.alt_elems * 4);
    L.spine = take(((size_t)sa::RADIX * sa::SORT_MAX_WG + sa::RADIX) * 4);
    L.status = take(((size_t)sa::ceil_div((int64_t)N1, sa::OS_MIN_TILE) + 1) * sa::RADIX * 8);
    L.err = take(256);
    L.starts = take(257 * 4);
    L.bitmap_bytes = ((N1 + 31) / 32 + 1) * 4;
    L.bitmap = take(L.bitmap_bytes);
    L.bytes = off;
    return L;
}

SA_EXPORT int64_t sa_amd_check_integrity_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)ci_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_check_integrity_device(const uint8_t *dT, int32_t n, const uint32_t *dSA, void *dWork,
                                                int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || (n > 0 && !dT)) return SA_AMD_EINVAL;
    if (work_bytes < ((int64_t)n + 1) * 4 + 256) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    using namespace sa;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *flags = (uint32_t *)dWork;
    uint32_t *rank = (uint32_t *)((char *)dWork + 256);
    HIP_TRY(hipMemsetAsync(flags, 0, 4, st));
    int64_t blocks = ((int64_t)n + 1 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    const CiLayout L = ci_layout(n);
    if (work_bytes >= (int64_t)L.bytes && (((uintptr_t)dWork) & 255u) == 0 && (((uintptr_t)dSA) & 15u) == 0 && n >= 2) {
        // ---- streaming form: range check, binned inverse permutation, one random rank line per slot ----
        hipLaunchKernelGGL(k_ci_range, dim3((unsigned)blocks), dim3(256), 0, st, dSA, (int64_t)n, flags);
        HIP_TRY(hipGetLastError());
        uint32_t f = 0;
        { const int rcw = read_words(&f, flags, 4, st); if (rcw) return rcw; }
        if (f & 1u) return SA_AMD_ERANGE;
        if (f & 2u) return 0;
        char *base = (char *)dWork;
        Workspace w;
        memset(&w, 0, sizeof(w));
        w.isa = (uint32_t *)(base + L.rank);
        w.spine = (uint32_t *)(base + L.spine);
        w.digit_tot = w.spine + (size_t)RADIX * SORT_MAX_WG;
        w.os_status = (unsigned long long *)(base + L.status);
        w.os_err = (uint32_t *)(base + L.err);
        w.ss.spine = w.spine; w.ss.digit_tot = w.digit_tot; w.ss.status = w.os_status; w.ss.err = w.os_err;
        HIP_TRY(hipMemsetAsync(w.os_err, 0, 16, st));
        uint32_t *alt = (uint32_t *)(base + L.alt);
        const Tuning tn = Tuning::from_env(N_SORT_VARIANTS, N_SORT32_VARIANTS, N_OS_SHAPES64, N_OS_SHAPES32);
        sa_amd_stats local;
        memset(&local, 0, sizeof(local));
        // pairs (SA[i], i), i = 0 .. n, binned by the suffix position; the scatter skips the empty suffix (value n)
        const int rcs = scatter_binned((uint32_t *)dSA, nullptr, alt, alt + L.alt_elems, (int64_t)n + 1, (int64_t)n, w, st, &local, tn, true,
                                       alt + 2 * L.alt_elems, alt + 3 * L.alt_elems);
        if (rcs) return rcs;
        // first bytes: boundaries proposed from the array, proved in text order (streaming); then the slot-order check
        uint32_t *starts = (uint32_t *)(base + L.starts), *bitmap = (uint32_t *)(base + L.bitmap);
        HIP_TRY(hipMemsetAsync(bitmap, 0, L.bitmap_bytes, st));
        hipLaunchKernelGGL(k_ci_starts, dim3(1), dim3(512), 0, st, dT, dSA, (int64_t)n, starts, bitmap);
        int64_t fblocks = ceil_div((int64_t)n, 256 * 16);
        if (fblocks > 16384) fblocks = 16384;
        hipLaunchKernelGGL(k_ci_first_bytes, dim3((unsigned)fblocks), dim3(256), 0, st, dT, (int64_t)n, (const uint32_t *)w.isa, (const uint32_t *)starts, flags);
        const int64_t cblocks = ceil_div((int64_t)n, (int64_t)CI_THREADS * CI_ITEMS);
        hipLaunchKernelGGL(k_ci_check_shared, dim3((unsigned)cblocks), dim3(CI_THREADS), 0, st, dSA, (int64_t)n, (const uint32_t *)w.isa,
                           (const uint32_t *)bitmap, flags);
        HIP_TRY(hipGetLastError());
        uint32_t words[2] = { 0, 0 };
        { const int rcw = read_words(&words[0], flags, 4, st); if (rcw) return rcw; }
        { const int rcw = read_words(&words[1], w.os_err, 4, st); if (rcw) return rcw; }
        if (words[1]) return SA_AMD_EINTERNAL;
        return (words[0] & 2u) ? 0 : 1;
    }
    // ---- small work block (4 (n + 1) + 256 bytes): random-store inverse, three rank reads per slot ----
    hipLaunchKernelGGL(sa::k_ci_scatter, dim3((unsigned)blocks), dim3(256), 0, st, dSA, (int64_t)n, rank, flags);
    hipLaunchKernelGGL(sa::k_ci_check, dim3((unsigned)blocks), dim3(256), 0, st, dT, dSA, (int64_t)n, (const uint32_t *)rank, flags);
    if (hipGetLastError() != hipSuccess) return SA_AMD_EHIP;
    uint32_t f = 0;
    if (hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return SA_AMD_EHIP;
    if (hipStreamSynchronize(st) != hipSuccess) return SA_AMD_EHIP;
    if (f & 1u) return SA_AMD_ERANGE;
    return (f & 2u) ? 0 : 1;
    SA_ABI_GUARD_END(0)
}

// enable_buckets on host buffers (reference src/sa.rs:89-119): the text goes up, 257 KiB come back; nothing else is needed --
// the reference builds the table from the text alone.
static int32_t bucket_table_host(const uint8_t *T, int32_t n, uint32_t *bkt)
{
    using namespace sa;
    if (n < 0 || !bkt || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (sa_amd_device_count() <= 0) return SA_AMD_ENODEVICE;
    const size_t tb = align_up((size_t)n + 16, 256);
    PooledScope sc(pick_device(), true);
    sc.acquire(tb + (size_t)BKT_LEN * 4);
    uint8_t *dT = (uint8_t *)sc.take(tb);
    uint32_t *dB = (uint32_t *)sc.take((size_t)BKT_LEN * 4);
    if (sc.rc == SA_AMD_OK && n > 0) sc.rc = hip_status(hipMemcpyAsync(dT, T, (size_t)n, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK) sc.rc = sa_amd_bucket_table_device(dT, nullptr, n, dB, sc.st);
    sc.down(bkt, dB, (size_t)BKT_LEN * 4);
    return sc.finish();
}

// host buffers; which = 2: integrity check, 3: build SA (into SA, n + 1 entries) then bucket table
static int32_t extras_host(const uint8_t *T, int32_t n, uint32_t *SA, int64_t sa_len, uint32_t *bkt, int which)
{
    using namespace sa;
    if (n < 0 || !SA || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (sa_amd_device_count() <= 0) return SA_AMD_ENODEVICE;
    if (which == 2 && sa_len != (int64_t)n + 1) return 0;          // reference src/sa.rs:73-75: false
    DeviceGuard guard(pick_device());
    if (guard.rc != SA_AMD_OK) return guard.rc;
    DevBuf dT, dSA, dB, dW;
    int32_t rc;
    const size_t N = (size_t)n;
    if ((rc = dT.alloc(N))) return rc;
    if ((rc = dSA.alloc((N + 1) * 4))) return rc;
    if (N) HIP_TRY(hipMemcpy(dT.p, T, N, hipMemcpyHostToDevice));
    if (which == 3) {
        const int64_t wb = sa_amd_workspace_bytes(n);
        if ((rc = dW.alloc((size_t)wb))) return rc;
        if ((rc = build_device(dT.as<uint8_t>(), dSA.as<uint32_t>(), n, dW.p, wb, nullptr, nullptr))) return rc;
        HIP_TRY(hipMemcpy(SA, dSA.p, (N + 1) * 4, hipMemcpyDeviceToHost));
        // the text is in HBM already: the table from its bigrams, as the reference counts them
        if ((rc = dB.alloc((size_t)BKT_LEN * 4))) return rc;
        if ((rc = sa_amd_bucket_table_device(dT.as<uint8_t>(), nullptr, n, dB.as<uint32_t>(), nullptr))) return rc;
        HIP_TRY(hipMemcpy(bkt, dB.p, (size_t)BKT_LEN * 4, hipMemcpyDeviceToHost));
        return SA_AMD_OK;
    }
    HIP_TRY(hipMemcpy(dSA.p, SA, (N + 1) * 4, hipMemcpyHostToDevice));
    int64_t wb = sa_amd_check_integrity_work_bytes(n);              // the streaming form; the small block if that much is not to be had
    rc = dW.alloc((size_t)wb);
    if (rc == SA_AMD_ENOMEM) { (void)hipGetLastError(); wb = ((int64_t)n + 1) * 4 + 256; rc = dW.alloc((size_t)wb); }
    if (rc) return rc;
    return sa_amd_check_integrity_device(dT.as<uint8_t>(), n, dSA.as<uint32_t>(), dW.p, wb, nullptr);
}

SA_EXPORT int32_t sa_amd_bucket_table(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *bkt)
{
    if (!bkt) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    (void)SA;                       // (the reference builds the table from the text alone, src/sa.rs:96-116)
    return bucket_table_host(T, n, bkt);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_saca_u8_buckets(const uint8_t *T, uint32_t *SA, int32_t n, uint32_t *bkt)
{
    if (!bkt) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return extras_host(T, n, SA, (int64_t)n + 1, bkt, 3);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_check_integrity(const uint8_t *T, int32_t n, const uint32_t *SA, int64_t sa_len)
{
    SA_ABI_GUARD_BEGIN
    return extras_host(T, n, (uint32_t *)SA, sa_len, nullptr, 2);
    SA_ABI_GUARD_END(0)
}

// ---- device-resident index: text + suffix array kept in HBM for bucket table, integrity check and batched search ----

struct sa_amd_index {
    int device;
    int32_t n;
    uint8_t *dT;
    uint32_t *dSA;
    uint32_t *dBkt;       // bucket table once sa_amd_index_buckets has built it (narrows the searches, src/sa.rs:123-161)
    uint64_t *dPair;      // LCP table of the search tree once sa_amd_index_enable_lcp has built it (kernels/esa.hpp)
    uint32_t *dDocOff;    // document offsets (ndocs + 1 entries) once sa_amd_index_set_documents has taken a collection (kernels/docs.hpp)
    uint32_t *dDocPrev;   // per slot: the previous slot of the same document + 1 (n + 1 entries)
    uint32_t ndocs;
    uint32_t *dDocSlots;  // the slots 1 .. n ordered by document once sa_amd_index_enable_doc_freq has built them (kernels/doc_tf.hpp)
};

SA_EXPORT int32_t sa_amd_index_create(const uint8_t *T, int32_t n, const uint32_t *SA, sa_amd_index **out)
{
    using namespace sa;
    if (!out || n < 0 || (n > 0 && !T)) return SA_AMD_EINVAL;
    *out = nullptr;
    if (sa_amd_device_count() <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    DeviceGuard guard(pick_device());
    if (guard.rc != SA_AMD_OK) return guard.rc;
    DevBuf dT, dSA;
    int32_t rc;
    const size_t N = (size_t)n;
    if ((rc = dT.alloc(N))) return rc;
    if ((rc = dSA.alloc((N + 1) * 4))) return rc;
    if (N) HIP_TRY(hipMemcpy(dT.p, T, N, hipMemcpyHostToDevice));
    if (SA) HIP_TRY(hipMemcpy(dSA.p, SA, (N + 1) * 4, hipMemcpyHostToDevice));
    else {                                                       // SuffixArray::new on the device
        DevBuf dW;
        const int64_t wb = sa_amd_workspace_bytes(n);
        if ((rc = dW.alloc((size_t)wb))) return rc;
        if ((rc = build_device(dT.as<uint8_t>(), dSA.as<uint32_t>(), n, dW.p, wb, nullptr, nullptr))) return rc;
    }
    sa_amd_index *ix = new (std::nothrow) sa_amd_index();
    if (!ix) return SA_AMD_ENOMEM;
    ix->n = n; ix->device = 0; ix->dBkt = nullptr; ix->dPair = nullptr;
    ix->dDocOff = nullptr; ix->dDocPrev = nullptr; ix->ndocs = 0; ix->dDocSlots = nullptr;
    (void)hipGetDevice(&ix->device);
    ix->dT = dT.as<uint8_t>(); ix->dSA = dSA.as<uint32_t>();
    dT.p = nullptr; dSA.p = nullptr;                             // ownership moves to the index
    *out = ix;
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_index_destroy(sa_amd_index *ix)      // (frees and deletes: nothing that throws)
{
    if (!ix) return;
    if (ix->dT) (void)hipFree(ix->dT);
    if (ix->dSA) (void)hipFree(ix->dSA);
    if (ix->dBkt) (void)hipFree(ix->dBkt);
    if (ix->dPair) (void)hipFree(ix->dPair);
    if (ix->dDocOff) (void)hipFree(ix->dDocOff);
    if (ix->dDocPrev) (void)hipFree(ix->dDocPrev);
    if (ix->dDocSlots) (void)hipFree(ix->dDocSlots);
    delete ix;
}

SA_EXPORT int32_t sa_amd_index_sa(const sa_amd_index *ix, uint32_t *SA_out)
{
    if (!ix || !SA_out) return SA_AMD_EINVAL;
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return hipMemcpy(SA_out, ix->dSA, ((size_t)ix->n + 1) * 4, hipMemcpyDeviceToHost) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

SA_EXPORT int32_t sa_amd_index_buckets(sa_amd_index *ix, uint32_t *bkt)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !bkt) return SA_AMD_EINVAL;
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    if (!ix->dBkt) {
        uint32_t *dB = nullptr;
        if (hipMalloc((void **)&dB, (size_t)sa::BKT_LEN * 4) != hipSuccess) { (void)hipGetLastError(); return SA_AMD_ENOMEM; }
        const int32_t rc = sa_amd_bucket_table_device(ix->dT, ix->dSA, ix->n, dB, nullptr);
        if (rc != SA_AMD_OK) { (void)hipFree(dB); return rc; }
        ix->dBkt = dB;                                           // kept: later searches start from the pattern's bucket
    }
    return hipMemcpy(bkt, ix->dBkt, (size_t)sa::BKT_LEN * 4, hipMemcpyDeviceToHost) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_check_integrity(const sa_amd_index *ix)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    // the work block of the streaming form comes from the process-wide pool (a 5.5 GB hipMalloc / hipFree per call would
    // cost more than the check); the small block if that much is not to be had
    sa::PooledScope sc(ix->device, false);
    int64_t wb = sa_amd_check_integrity_work_bytes(ix->n);
    if (sc.acquire((size_t)wb) == SA_AMD_ENOMEM) { wb = ((int64_t)ix->n + 1) * 4 + 256; sc.acquire_smaller((size_t)wb); }
    if (sc.rc) return sc.rc;
    const int32_t ok = sa_amd_check_integrity_device(ix->dT, ix->n, ix->dSA, sc.take((size_t)wb), wb, nullptr);      // 1 / 0, or a code
    if (ok < 0) sc.rc = ok;
    (void)sc.finish();
    return ok;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_search(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count,
                                      uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi, uint32_t *lcp_start,
                                      uint32_t *lcp_len)
{
    SA_ABI_GUARD_BEGIN
    using namespace sa;
    if (!ix || !search_patterns_valid(pat_data, pat_off, count)) return SA_AMD_EINVAL;
    if (count == 0) {
        sa_amd_search_stats z;
        memset(&z, 0, sizeof(z));
        z.route = ix->dPair ? 1 : 0;
        if (!ix->dPair) z.compared_bytes = z.steps = z.table_steps = -1;
        g_last_search_stats = z;
        return SA_AMD_OK;
    }
    const int64_t total = pat_off[count];
    DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    const size_t C = (size_t)count;
    DevBuf dP, dO, dC, dR;
    int32_t rc;
    if ((rc = dP.alloc((size_t)total))) return rc;
    if ((rc = dO.alloc((C + 1) * 8))) return rc;
    if ((rc = dC.alloc(C))) return rc;
    if ((rc = dR.alloc(C * 4 * 4))) return rc;
    if (total) HIP_TRY(hipMemcpy(dP.p, pat_data, (size_t)total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dO.p, pat_off, (C + 1) * 8, hipMemcpyHostToDevice));
    uint32_t *R = dR.as<uint32_t>();
    sa_amd_search_stats stats;
    memset(&stats, 0, sizeof(stats));
    stats.patterns = count;
    stats.compared_bytes = stats.steps = stats.table_steps = -1;
    DevBuf dS;
    if (ix->dPair) {                                             // LCP route (kernels/esa.hpp): its three counters
        if ((rc = dS.alloc(3 * 8))) return rc;
        HIP_TRY(hipMemset(dS.p, 0, 3 * 8));
    }
    if ((rc = launch_search(ix->dT, ix->dSA, ix->n, ix->dBkt, ix->dPair, dP.as<const uint8_t>(), dO.as<const int64_t>(), count, dC.as<uint8_t>(), R, R + C,
                            R + 2 * C, R + 3 * C, ix->dPair ? dS.as<unsigned long long>() : nullptr, nullptr))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (ix->dPair) {
        int64_t cw[3];
        HIP_TRY(hipMemcpy(cw, dS.p, sizeof(cw), hipMemcpyDeviceToHost));
        stats.compared_bytes = cw[0]; stats.steps = cw[1]; stats.table_steps = cw[2];
        stats.route = 1;
    }
    g_last_search_stats = stats;
    if (contains) HIP_TRY(hipMemcpy(contains, dC.p, C, hipMemcpyDeviceToHost));
    if (range_lo) HIP_TRY(hipMemcpy(range_lo, R, C * 4, hipMemcpyDeviceToHost));
    if (range_hi) HIP_TRY(hipMemcpy(range_hi, R + C, C * 4, hipMemcpyDeviceToHost));
    if (lcp_start) HIP_TRY(hipMemcpy(lcp_start, R + 2 * C, C * 4, hipMemcpyDeviceToHost));
    if (lcp_len) HIP_TRY(hipMemcpy(lcp_len, R + 3 * C, C * 4, hipMemcpyDeviceToHost));
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

// ---- LCP array (host/lcp.hpp, kernels/lcp.hpp) ----

SA_EXPORT int64_t sa_amd_lcp_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::lcp_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_lcp_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dLCP, void *dWork,
                                    int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dLCP || !dWork || (n > 0 && !dT)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::lcp_device(dT, dSA, n, dLCP, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_lcp(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *LCP)
{
    SA_ABI_GUARD_BEGIN
    return sa::lcp_host(T, n, (uint32_t *)SA, LCP, false);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_saca_u8_lcp(const uint8_t *T, uint32_t *SA, int32_t n, uint32_t *LCP)
{
    SA_ABI_GUARD_BEGIN
    return sa::lcp_host(T, n, SA, LCP, true);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_lcp(const sa_amd_index *ix, uint32_t *LCP)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !LCP) return SA_AMD_EINVAL;
    const size_t lb = ((size_t)ix->n + 1) * 4;
    sa::PooledScope sc(ix->device, false);
    const sa::Inputs in = sa::resident_inputs(sc, ix->dT, ix->dSA, sa::lcp_layout(ix->n).bytes, lb);
    uint32_t *dL = (uint32_t *)sc.take(lb);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::lcp_device(in.dT, in.dSA, ix->n, dL, in.dW, (int64_t)in.wb, sc.st);
    sc.down(LCP, dL, lb);
    return sc.finish();
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_enable_lcp(sa_amd_index *ix)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    if (ix->dPair) return SA_AMD_OK;
    sa::PooledScope sc(ix->device, false);
    if (sc.rc) return sc.rc;
    sa::DevBuf pair;                                             // the table outlives the call: its own allocation, not the pool's
    if (pair.alloc(((size_t)ix->n + 1) * 8) != SA_AMD_OK) { (void)hipGetLastError(); return SA_AMD_ENOMEM; }      // (the refused allocation's error is cleared, as everywhere)
    // LCP array and its work block from the pool, as sa_amd_index_lcp; the tile minima of the table build behind them
    const size_t lb = sa::align_up(((size_t)ix->n + 1) * 4, 256), mb = sa::esa_mins_elems(ix->n) * 4;
    const sa::Inputs in = sa::resident_inputs(sc, ix->dT, ix->dSA, sa::lcp_layout(ix->n).bytes, lb + mb);
    uint32_t *dL = (uint32_t *)sc.take(lb), *dMins = (uint32_t *)sc.take(mb);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::lcp_device(in.dT, in.dSA, ix->n, dL, in.dW, (int64_t)in.wb, sc.st);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::esa_build(dL, ix->n, pair.as<uint64_t>(), dMins, sc.st);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::hip_status(hipDeviceSynchronize());      // (the route's own wait: finish() adds none on success)
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    ix->dPair = pair.as<uint64_t>();                             // kept: later searches take the LCP route
    pair.p = nullptr;
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_search_stats(sa_amd_search_stats *out)
{
    if (out) *out = sa::g_last_search_stats;
}

SA_EXPORT int32_t sa_amd_lcp_set_compare_cap(int32_t bytes)
{
    const int32_t prev = sa::g_lcp_cap < 0 ? sa::LCP_CAP_DEFAULT : sa::g_lcp_cap;
    sa::g_lcp_cap = bytes < 0 ? -1 : (bytes > sa::LCP_CAP_MAX ? sa::LCP_CAP_MAX : bytes);
    return prev;
}

SA_EXPORT void sa_amd_last_lcp_stats(sa_amd_lcp_stats *out)
{
    if (out) *out = sa::g_last_lcp_stats;
}

// ---- Burrows-Wheeler transform and its inverse (host/bwt.hpp, kernels/bwt.hpp) ----

SA_EXPORT int64_t sa_amd_bwt_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::BWT_WORK_BYTES;
}

SA_EXPORT int32_t sa_amd_bwt_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint8_t *dBWT, int32_t *primary_out,
                                    void *dWork, int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !primary_out || !dWork || (n > 0 && (!dT || !dBWT))) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::bwt_device(dT, dSA, n, dBWT, primary_out, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_bwt(const uint8_t *T, int32_t n, const uint32_t *SA, uint8_t *BWT, int32_t *primary_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::bwt_host(T, n, SA, BWT, primary_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_bwt(const sa_amd_index *ix, uint8_t *BWT, int32_t *primary_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !primary_out || (ix->n > 0 && !BWT)) return SA_AMD_EINVAL;
    sa::PooledScope sc(ix->device, false);
    const sa::Inputs in = sa::resident_inputs(sc, ix->dT, ix->dSA, sa::BWT_WORK_BYTES, (size_t)ix->n + 16);
    return sa::bwt_resident(sc, in, ix->n, BWT, primary_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int64_t sa_amd_unbwt_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::unbwt_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_unbwt_device(const uint8_t *dBWT, int32_t n, int32_t primary, uint8_t *dT_out, void *dWork,
                                      int64_t work_bytes, void *stream)
{
    if (n < 0 || (n > 0 && (!dBWT || !dT_out || !dWork))) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::unbwt_device(dBWT, n, primary, dT_out, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_unbwt(const uint8_t *BWT, int32_t n, int32_t primary, uint8_t *T_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::unbwt_host(BWT, n, primary, T_out);
    SA_ABI_GUARD_END(0)
}

// ---- repeat finding (host/repeats.hpp, kernels/repeats.hpp) ----

SA_EXPORT int64_t sa_amd_repeats_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::rep_layout(n).bytes;
}

SA_EXPORT int64_t sa_amd_repeat_spans_bound(int32_t n, int32_t min_len)
{
    if (n < 0 || min_len < 1) return -1;
    return sa::repeat_spans_bound(n, min_len);
}

SA_EXPORT int32_t sa_amd_repeat_lengths_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dLR, void *dWork,
                                               int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || (n > 0 && (!dT || !dLR))) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::repeats_device(dT, dSA, n, false, dLR, 1, 0, nullptr, 0, nullptr, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_repeat_spans_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, int32_t min_len, int32_t mode,
                                             uint32_t *dSpans, int64_t capacity, int64_t *count_out, void *dWork,
                                             int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || !count_out || (n > 0 && !dT) || (capacity > 0 && !dSpans)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::repeats_device(dT, dSA, n, true, nullptr, min_len, mode, dSpans, capacity, count_out, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_repeat_lengths(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *LR)
{
    if (n > 0 && !LR) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::repeats_host(T, n, SA, false, LR, 1, 0, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_repeat_spans(const uint8_t *T, int32_t n, const uint32_t *SA, int32_t min_len, int32_t mode, uint32_t *spans,
                                      int64_t capacity, int64_t *count_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::repeats_host(T, n, SA, true, nullptr, min_len, mode, spans, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

// the index's resident text and array: only the work block and the output come from the pool; on the null stream
static int32_t index_repeats(const sa_amd_index *ix, bool spans, uint32_t *LR, int32_t min_len, int32_t mode, uint32_t *out_spans,
                             int64_t capacity, int64_t *count_out)
{
    if (!ix) return SA_AMD_EINVAL;
    if (spans ? (min_len < 1 || (mode != SA_AMD_REPEATS_ALL && mode != SA_AMD_REPEATS_KEEP_FIRST) || capacity < 0 || !count_out ||
                 (capacity > 0 && !out_spans))
              : (ix->n > 0 && !LR)) return SA_AMD_EINVAL;
    sa::CappedRows rows;
    if (spans) rows = sa::CappedRows(capacity, sa::repeat_spans_bound(ix->n, min_len));
    sa::PooledScope sc(ix->device, false);
    const sa::Inputs in = sa::resident_inputs(sc, ix->dT, ix->dSA, sa::rep_layout(ix->n).bytes, spans ? rows.bytes() : ((size_t)ix->n + 1) * 4);
    return sa::repeats_resident(sc, in, ix->n, spans, LR, min_len, mode, out_spans, rows, count_out);
}

SA_EXPORT int32_t sa_amd_index_repeat_lengths(const sa_amd_index *ix, uint32_t *LR)
{
    SA_ABI_GUARD_BEGIN
    return index_repeats(ix, false, LR, 1, 0, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_repeat_spans(const sa_amd_index *ix, int32_t min_len, int32_t mode, uint32_t *spans, int64_t capacity,
                                            int64_t *count_out)
{
    SA_ABI_GUARD_BEGIN
    return index_repeats(ix, true, nullptr, min_len, mode, spans, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_repeat_stats(sa_amd_repeat_stats *out)
{
    if (out) *out = sa::g_last_repeat_stats;
}

// ---- Lempel-Ziv factorisation (host/lz.hpp, kernels/lz.hpp) ----

SA_EXPORT int64_t sa_amd_lz_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::lz_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_lpf_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dLPF, uint32_t *dSRC, void *dWork,
                                    int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || (n > 0 && !dT)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::lz_device(dT, dSA, n, false, dLPF, dSRC, nullptr, 0, nullptr, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_lz77_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dPhrases, int64_t capacity,
                                     int64_t *count_out, void *dWork, int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || !count_out || (n > 0 && !dT) || (capacity > 0 && !dPhrases)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::lz_device(dT, dSA, n, true, nullptr, nullptr, dPhrases, capacity, count_out, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_lpf(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *LPF, uint32_t *SRC)
{
    SA_ABI_GUARD_BEGIN
    return sa::lz_host(T, n, SA, false, LPF, SRC, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_lz77(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *phrases, int64_t capacity, int64_t *count_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::lz_host(T, n, SA, true, nullptr, nullptr, phrases, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

// the index's resident text and array: only the work block and the outputs come from the pool; on the null stream
static int32_t index_lz(const sa_amd_index *ix, bool parse, uint32_t *LPF, uint32_t *SRC, uint32_t *phrases, int64_t capacity, int64_t *count_out)
{
    if (!ix) return SA_AMD_EINVAL;
    if (parse && (capacity < 0 || !count_out || (capacity > 0 && !phrases))) return SA_AMD_EINVAL;
    sa::CappedRows rows;
    if (parse) rows = sa::CappedRows(capacity, ix->n);
    sa::PooledScope sc(ix->device, false);
    const sa::Inputs in = sa::resident_inputs(sc, ix->dT, ix->dSA, sa::lz_layout(ix->n).bytes,
                                              parse ? rows.bytes() : 2 * sa::align_up(((size_t)ix->n + 1) * 4, 256));
    return sa::lz_resident(sc, in, ix->n, parse, LPF, SRC, phrases, rows, count_out);
}

SA_EXPORT int32_t sa_amd_index_lpf(const sa_amd_index *ix, uint32_t *LPF, uint32_t *SRC)
{
    SA_ABI_GUARD_BEGIN
    return index_lz(ix, false, LPF, SRC, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_lz77(const sa_amd_index *ix, uint32_t *phrases, int64_t capacity, int64_t *count_out)
{
    SA_ABI_GUARD_BEGIN
    return index_lz(ix, true, nullptr, nullptr, phrases, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_lz_stats(sa_amd_lz_stats *out)
{
    if (out) *out = sa::g_last_lz_stats;
}

// ---- matching statistics and shared spans of a query against the index (host/match.hpp, kernels/match.hpp) ----

static sa::MatchIndex match_index(const sa_amd_index *ix)
{
    sa::MatchIndex mi;
    mi.dT = ix->dT; mi.dSA = ix->dSA; mi.n = ix->n; mi.dBkt = ix->dBkt; mi.dPair = ix->dPair;
    return mi;
}

SA_EXPORT int64_t sa_amd_match_work_bytes(int32_t m)
{
    if (m < 0) return -1;
    return (int64_t)sa::match_layout(m).bytes;
}

SA_EXPORT int32_t sa_amd_index_match_stats(const sa_amd_index *ix, const uint8_t *Q, int32_t m, int32_t max_len, uint32_t *ML, uint32_t *POS)
{
    if (!ix || m < 0 || max_len < 1 || (m > 0 && !Q)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_host(match_index(ix), Q, m, max_len, false, ML, POS, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_match_stats_device(const sa_amd_index *ix, const uint8_t *dQ, int32_t m, int32_t max_len, uint32_t *dML,
                                                  uint32_t *dPOS, void *dWork, int64_t work_bytes, void *stream)
{
    if (!ix || m < 0 || max_len < 1 || (m > 0 && !dQ)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_device(match_index(ix), dQ, m, max_len, false, dML, dPOS, nullptr, 0, nullptr, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_match_spans(const sa_amd_index *ix, const uint8_t *Q, int32_t m, int32_t min_len, uint32_t *spans,
                                           int64_t capacity, int64_t *count_out)
{
    if (!ix || m < 0 || min_len < 1 || (m > 0 && !Q) || capacity < 0 || !count_out || (capacity > 0 && !spans)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_host(match_index(ix), Q, m, min_len, true, nullptr, nullptr, spans, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_match_spans_device(const sa_amd_index *ix, const uint8_t *dQ, int32_t m, int32_t min_len, uint32_t *dSpans,
                                                  int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes, void *stream)
{
    if (!ix || m < 0 || min_len < 1 || (m > 0 && !dQ) || capacity < 0 || !count_out || (capacity > 0 && !dSpans)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_device(match_index(ix), dQ, m, min_len, true, nullptr, nullptr, dSpans, capacity, count_out, dWork, work_bytes,
                            (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_match_stats(sa_amd_match_stats *out)
{
    if (out) *out = sa::g_last_match_stats;
}

SA_EXPORT int32_t sa_amd_match_set_group_cap(int32_t bytes)
{
    const int32_t prev = sa::g_match_cap < 0 ? sa::MATCH_CAP_DEFAULT : sa::g_match_cap;
    sa::g_match_cap = bytes < 0 ? -1 : (bytes > sa::MATCH_CAP_MAX ? sa::MATCH_CAP_MAX : bytes);
    return prev;
}

SA_EXPORT int32_t sa_amd_match_set_group_lanes(int32_t lanes)
{
    const int32_t prev = sa::g_match_lanes;
    sa::g_match_lanes = lanes < 0 ? 8 : (lanes >= 16 ? 16 : (lanes >= 8 ? 8 : 4));
    return prev;
}

// ---- document collections over the index (host/docs.hpp, kernels/docs.hpp) ----

static sa::DocIndex doc_index(const sa_amd_index *ix)
{
    sa::DocIndex di;
    di.device = ix->device; di.dT = ix->dT; di.dSA = ix->dSA; di.n = ix->n; di.dBkt = ix->dBkt; di.dPair = ix->dPair;
    di.dOff = ix->dDocOff; di.dPrev = ix->dDocPrev; di.ndocs = ix->ndocs; di.dSlots = ix->dDocSlots;
    return di;
}

SA_EXPORT int64_t sa_amd_docs_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::docs_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_index_set_documents(sa_amd_index *ix, const uint32_t *doc_off, int64_t ndocs)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::docs_valid(doc_off, ndocs) || doc_off[ndocs] != (uint32_t)ix->n) return SA_AMD_EINVAL;
    const size_t M = (size_t)ndocs + 1, N1 = (size_t)ix->n + 1;
    sa::PooledScope sc(ix->device, false);
    if (sc.rc) return sc.rc;
    sa::DevBuf off, prev;                                        // the tables outlive the call: their own allocations, not the pool's
    if (off.alloc(M * 4) != SA_AMD_OK || prev.alloc(N1 * 4) != SA_AMD_OK) { (void)hipGetLastError(); return SA_AMD_ENOMEM; }
    const size_t wb = sa::docs_layout(ix->n).bytes;
    sc.acquire(wb);
    void *dW = sc.take(wb);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::hip_status(hipMemcpy(off.p, doc_off, M * 4, hipMemcpyHostToDevice));
    if (sc.rc == SA_AMD_OK) sc.rc = sa::docs_build(ix->dSA, ix->n, off.as<uint32_t>(), (uint32_t)ndocs, prev.as<uint32_t>(), dW, (int64_t)wb, sc.st);
    if (sc.finish() != SA_AMD_OK) return sc.rc;                  // (a previous collection stays)
    if (ix->dDocOff) (void)hipFree(ix->dDocOff);
    if (ix->dDocPrev) (void)hipFree(ix->dDocPrev);
    if (ix->dDocSlots) (void)hipFree(ix->dDocSlots);             // the frequency table was the old collection's: enabled again by the caller
    ix->dDocSlots = nullptr;
    ix->dDocOff = off.as<uint32_t>(); ix->dDocPrev = prev.as<uint32_t>(); ix->ndocs = (uint32_t)ndocs;
    off.p = nullptr; prev.p = nullptr;
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_of(const sa_amd_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || count < 0 || (count > 0 && (!pos || !doc_out)) || !ix->dDocOff) return SA_AMD_EINVAL;
    if (count == 0) return SA_AMD_OK;
    const size_t b = sa::align_up((size_t)count * 4, 256);
    sa::PooledScope sc(ix->device, false);
    sc.acquire(2 * b);
    uint32_t *dPos = (uint32_t *)sc.take(b), *dOut = (uint32_t *)sc.take(b);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::hip_status(hipMemcpyAsync(dPos, pos, (size_t)count * 4, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK) sc.rc = sa::launch_doc_of(dPos, count, ix->dDocOff, ix->ndocs, ix->n, dOut, sc.st);
    sc.down(doc_out, dOut, (size_t)count * 4);
    return sc.finish();
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_of_device(const sa_amd_index *ix, const uint32_t *dPos, int64_t count, uint32_t *dDoc, void *stream)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || count < 0 || (count > 0 && (!dPos || !dDoc)) || ((((uintptr_t)dPos) | ((uintptr_t)dDoc)) & 3u) || !ix->dDocOff) return SA_AMD_EINVAL;
    if (count == 0) return SA_AMD_OK;
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    const int32_t rc = sa::launch_doc_of(dPos, count, ix->dDocOff, ix->ndocs, ix->n, dDoc, (hipStream_t)stream);
    if (rc) return rc;
    return sa::hip_status(hipStreamSynchronize((hipStream_t)stream));
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_search(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, uint32_t *occ,
                                          uint32_t *df)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count) || !ix->dDocOff) return SA_AMD_EINVAL;
    return sa::docs_query(doc_index(ix), pat_data, pat_off, count, false, occ, df, nullptr, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_list(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int64_t *list_off,
                                        uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count)) return SA_AMD_EINVAL;
    if (capacity < 0 || !list_off || !total_out || (capacity > 0 && !docs) || !ix->dDocOff) return SA_AMD_EINVAL;
    return sa::docs_query(doc_index(ix), pat_data, pat_off, count, true, nullptr, nullptr, list_off, docs, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_docs_stats(sa_amd_docs_stats *out)
{
    if (out) *out = sa::g_last_docs_stats;
}

SA_EXPORT int32_t sa_amd_docs_set_chunk(int32_t slots)
{
    const int32_t prev = sa::g_docs_chunk < 0 ? sa::DOC_CHUNK_DEFAULT : sa::g_docs_chunk;
    sa::g_docs_chunk = slots < 0 ? -1 : (slots < sa::DOC_CHUNK_MIN ? sa::DOC_CHUNK_MIN : (slots > sa::DOC_CHUNK_MAX ? sa::DOC_CHUNK_MAX : slots));
    return prev;
}

// ---- document-aware duplicate spans (host/doc_repeats.hpp, kernels/doc_repeats.hpp) ----

SA_EXPORT int64_t sa_amd_doc_repeats_work_bytes(int32_t n, int64_t ndocs)
{
    if (n < 0 || ndocs < 1 || ndocs > (int64_t)0xfffffffe) return -1;
    return (int64_t)sa::docrep_layout(n, ndocs).bytes;
}

SA_EXPORT int32_t sa_amd_index_doc_repeat_spans(const sa_amd_index *ix, int32_t min_len, int32_t mode, int32_t scope, uint32_t *spans,
                                                int64_t capacity, int64_t *count_out, uint32_t *doc_bytes)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !ix->dDocOff || !sa::docrep_args_valid(min_len, mode, scope, spans, capacity, count_out)) return SA_AMD_EINVAL;
    return sa::doc_repeats_index(doc_index(ix), min_len, mode, scope, spans, capacity, count_out, doc_bytes);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_doc_repeat_stats(sa_amd_doc_repeat_stats *out)
{
    if (out) *out = sa::g_last_doc_repeat_stats;
}

// ---- per-document term frequencies and top-k documents (host/doc_tf.hpp, kernels/doc_tf.hpp) ----

SA_EXPORT int32_t sa_amd_index_enable_doc_freq(sa_amd_index *ix)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !ix->dDocOff) return SA_AMD_EINVAL;
    if (ix->dDocSlots) return SA_AMD_OK;
    sa::PooledScope sc(ix->device, false);
    if (sc.rc) return sc.rc;
    sa::DevBuf slots;                                            // the table outlives the call: its own allocation, not the pool's
    if (slots.alloc(((size_t)ix->n + 1) * 4) != SA_AMD_OK) { (void)hipGetLastError(); return SA_AMD_ENOMEM; }      // (n entries; never empty)
    const size_t wb = sa::docs_layout(ix->n).bytes;
    sc.acquire(wb);
    void *dW = sc.take(wb);
    if (sc.rc == SA_AMD_OK) sc.rc = sa::docs_freq_build(ix->dSA, ix->n, ix->dDocOff, ix->ndocs, slots.as<uint32_t>(), dW, (int64_t)wb, sc.st);
    if (sc.finish() != SA_AMD_OK) return sc.rc;
    ix->dDocSlots = slots.as<uint32_t>();
    slots.p = nullptr;
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_tf(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int64_t *list_off,
                                      uint32_t *docs, uint32_t *tf, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    // (in this order: everything that can be refused without the index is, before the index is looked at)
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count) || capacity < 0 || !list_off || !total_out) return SA_AMD_EINVAL;
    if (!ix->dDocOff || !ix->dDocSlots) return SA_AMD_EINVAL;
    return sa::doc_tf_query(doc_index(ix), pat_data, pat_off, count, 0, list_off, docs, tf, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_topk(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int32_t k,
                                        int64_t *top_off, uint32_t *docs, uint32_t *tf)
{
    SA_ABI_GUARD_BEGIN
    // (in this order: everything that can be refused without the index is, before the index is looked at)
    if (!ix || k < 1 || k > SA_AMD_DOC_TOPK_MAX || !sa::search_patterns_valid(pat_data, pat_off, count) || !top_off) return SA_AMD_EINVAL;
    if (!ix->dDocOff || !ix->dDocSlots) return SA_AMD_EINVAL;
    return sa::doc_tf_query(doc_index(ix), pat_data, pat_off, count, k, top_off, docs, tf, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_doc_tf_stats(sa_amd_doc_tf_stats *out)
{
    if (out) *out = sa::g_last_doc_tf_stats;
}

SA_EXPORT int32_t sa_amd_docs_set_topk_piece(int32_t entries)
{
    const int32_t prev = sa::g_topk_piece < 0 ? sa::DOC_TOPK_PIECE_DEFAULT : sa::g_topk_piece;
    const int32_t e = entries < sa::DOC_TOPK_PIECE_MIN ? sa::DOC_TOPK_PIECE_MIN : (entries > sa::DOC_TOPK_PIECE_MAX ? sa::DOC_TOPK_PIECE_MAX : entries);
    sa::g_topk_piece = entries < 0 ? -1 : (int32_t)sa::topk_pow2_floor((uint32_t)e);
    return prev;
}

SA_EXPORT void sa_amd_last_unbwt_stats(sa_amd_unbwt_stats *out)
{
    if (out) *out = sa::g_last_unbwt_stats;
}

SA_EXPORT void sa_amd_unbwt_set_walk_limits(int32_t cap_steps, int32_t max_launches)
{
    sa::g_unbwt_cap = cap_steps < 0 ? -1 : (cap_steps < 1 ? 1 : (cap_steps > sa::UNBWT_CAP_MAX ? sa::UNBWT_CAP_MAX : cap_steps));
    sa::g_unbwt_launches = max_launches < 0 ? -1 : (max_launches < 1 ? 1 : max_launches);
}

SA_EXPORT int32_t sa_amd_unbwt_set_splitter_spacing(int32_t spacing)
{
    const int32_t prev = sa::g_unbwt_spacing < 0 ? sa::UNBWT_SPACING_DEFAULT : sa::g_unbwt_spacing;
    if (spacing < 0) { sa::g_unbwt_spacing = -1; return prev; }
    int32_t s = sa::UNBWT_SPACING_MIN;                       // rounded down to a power of two inside the range
    while (s * 2 <= spacing && s < sa::UNBWT_SPACING_MAX) s *= 2;
    sa::g_unbwt_spacing = s;
    return prev;
}

// ---- packed format (reference src/packed_sa.rs); byte layout: u32 magic "SA4x" LE, u32 length, u64 data length
//      (bincode's Vec<u8> prefix), data ----

static int sa_bits_of(uint32_t length)          // reference src/packed_sa.rs:127-129
{
    const uint32_t v = length ? length - 1 : 0;
    return v ? sa::bit_length(v) : 0;
}

SA_EXPORT int64_t sa_amd_pack_bound(int64_t length)
{
    if (length < 0 || length > 0xffffffffLL) return -1;
    const int bits = sa_bits_of((uint32_t)length);
    return 16 + (int64_t)((length + 127) / 128) * bits * 16;
}

SA_EXPORT int32_t sa_amd_pack(const uint32_t *SA, int64_t length, uint8_t *out, int64_t capacity, int64_t *out_len)
{
    SA_ABI_GUARD_BEGIN
    using namespace sa;
    if (!SA || !out || !out_len || length < 1 || length > 0xffffffffLL) return SA_AMD_EINVAL;
    if (capacity < sa_amd_pack_bound(length)) return SA_AMD_EINVAL;
    if (sa_amd_device_count() <= 0) return SA_AMD_ENODEVICE;
    const int bits = sa_bits_of((uint32_t)length);
    const int64_t blocks = (length + 127) / 128;
    const int64_t words = blocks * bits * 4;
    int64_t data_len = 0;
    if (bits > 0) {
        DeviceGuard guard(pick_device());
        if (guard.rc != SA_AMD_OK) return guard.rc;
        DevBuf dS, dO;
        int32_t rc;
        if ((rc = dS.alloc((size_t)length * 4))) return rc;
        if ((rc = dO.alloc((size_t)words * 4))) return rc;
        HIP_TRY(hipMemcpy(dS.p, SA, (size_t)length * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_pack4x, dim3((unsigned)ceil_div(words, 256)), dim3(256), 0, nullptr, dS.as<const uint32_t>(), length, bits,
                           dO.as<uint32_t>(), words);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + 16, dO.p, (size_t)words * 4, hipMemcpyDeviceToHost));
        data_len = words * 4;
        if (length % 128) {                                   // a partial last block loses its trailing zero bytes (src/packed_sa.rs:41-45)
            const int64_t last = (blocks - 1) * bits * 16;
            while (data_len > last && out[16 + data_len - 1] == 0) --data_len;
        }
    }
    const uint32_t magic = 2016690515u, len32 = (uint32_t)length;   // src/packed_sa.rs:7
    const uint64_t dl = (uint64_t)data_len;
    memcpy(out, &magic, 4); memcpy(out + 4, &len32, 4); memcpy(out + 8, &dl, 8);
    *out_len = 16 + data_len;
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_unpack(const uint8_t *bytes, int64_t nbytes, uint32_t *SA, int64_t capacity, int64_t *length)
{
    SA_ABI_GUARD_BEGIN
    using namespace sa;
    if (!bytes || !length || nbytes < 16) return SA_AMD_EINVAL;
    uint32_t magic, len32; uint64_t dl;
    memcpy(&magic, bytes, 4); memcpy(&len32, bytes + 4, 4); memcpy(&dl, bytes + 8, 8);
    if (magic != 2016690515u || dl != (uint64_t)(nbytes - 16)) return SA_AMD_EINVAL;       // InvalidData in the reference
    *length = len32;
    if (!SA || capacity < (int64_t)len32) return SA_AMD_EINVAL;
    const int bits = sa_bits_of(len32);
    const int64_t blocks = ((int64_t)len32 + 127) / 128;
    const int64_t full = blocks * bits * 16;
    // every block but the last is stored whole, and only a PARTIAL last block is right-trimmed (src/packed_sa.rs:36-46):
    // anything shorter is a truncated file, not an array with missing zeros
    const int64_t min_dl = (len32 % 128) ? (blocks - 1) * bits * 16 : full;
    if ((int64_t)dl > full || (int64_t)dl < min_dl) return SA_AMD_EINVAL;
    if (len32 == 0) return SA_AMD_OK;
    if (bits == 0) { SA[0] = 0; return SA_AMD_OK; }           // length 1: the reference's unpack loop does not terminate here
    if (sa_amd_device_count() <= 0) return SA_AMD_ENODEVICE;
    DeviceGuard guard(pick_device());
    if (guard.rc != SA_AMD_OK) return guard.rc;
    const int64_t in_words = ((int64_t)dl + 3) / 4;
    DevBuf dI, dS;
    int32_t rc;
    if ((rc = dI.alloc((size_t)(in_words ? in_words : 1) * 4))) return rc;
    if ((rc = dS.alloc((size_t)len32 * 4))) return rc;
    HIP_TRY(hipMemset(dI.p, 0, (size_t)(in_words ? in_words : 1) * 4));
    if (dl) HIP_TRY(hipMemcpy(dI.p, bytes + 16, (size_t)dl, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_unpack4x, dim3((unsigned)ceil_div((int64_t)len32, 256)), dim3(256), 0, nullptr, dI.as<const uint32_t>(), in_words,
                       (int64_t)len32, bits, dS.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(SA, dS.p, (size_t)len32 * 4, hipMemcpyDeviceToHost));
    return SA_AMD_OK;
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_release_cache(void)
{
    try { sa::pool().clear(); } catch (...) { }
}

SA_EXPORT void sa_amd_last_stats(sa_amd_stats *out)
{
    if (out) *out = sa::g_last_stats;
}

SA_EXPORT int32_t sa_amd_last_host_timing(double *ms, int32_t capacity)
{
    const sa::HostTiming &t = sa::g_host_timing;
    const double v[9] = { t.acquire, t.h2d, t.build, t.d2h, t.release, t.total, (double)t.staged, t.early, t.spill };
    for (int i = 0; i < capacity && i < 9; ++i) ms[i] = v[i];
    return 9;
}

SA_EXPORT int32_t sa_amd_device_count(void)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    return ndev;
}

SA_EXPORT int32_t sa_amd_device_pci_bus_id(int32_t device, char *buf, int32_t capacity)
{
    if (!buf || capacity < 16) return SA_AMD_EINVAL;
    buf[0] = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SA_AMD_ENODEVICE;
    if (device < 0 || device >= ndev) return SA_AMD_EINVAL;
    if (hipDeviceGetPCIBusId(buf, capacity, device) != hipSuccess) { (void)hipGetLastError(); buf[0] = 0; return SA_AMD_EHIP; }
    return SA_AMD_OK;
}

SA_EXPORT const char *sa_amd_strerror(int32_t code)
{
    switch (code) {
    case SA_AMD_OK: return "ok";
    case SA_AMD_EINVAL: return "invalid argument";
    case SA_AMD_ENOMEM: return "out of memory";
    case SA_AMD_EHIP: return "HIP runtime error";
    case SA_AMD_ENODEVICE: return "no HIP device";
    case SA_AMD_EINTERNAL: return "internal error: refinement did not converge";
    case SA_AMD_ERANGE: return "suffix offset out of range";
    default: return "unknown error";
    }
}

SA_EXPORT void sa_amd_profile_begin_classes(uint64_t class_mask)
{
    sa::Profiler &p = sa::g_prof;
    p.on = true;
    p.mask = class_mask;
    for (int i = 0; i < sa::KC_COUNT; ++i) { p.ms[i] = 0; p.launches[i] = 0; p.units[i] = 0; }
}

SA_EXPORT void sa_amd_profile_begin(void) { sa_amd_profile_begin_classes(~0ull); }

SA_EXPORT int32_t sa_amd_profile_end(double *ms, int64_t *launches, int64_t *units, int32_t capacity)
{
    sa::Profiler &p = sa::g_prof;
    p.on = false;
    const int cnt = capacity < sa::KC_COUNT ? capacity : sa::KC_COUNT;
    for (int i = 0; i < cnt; ++i) {
        if (ms) ms[i] = p.ms[i];
        if (launches) launches[i] = p.launches[i];
        if (units) units[i] = p.units[i];
    }
    return sa::KC_COUNT;
}

SA_EXPORT const char *sa_amd_profile_kernel_name(int32_t i)
{
    return (i >= 0 && i < sa::KC_COUNT) ? sa::kclass_names[i] : "";
}

#ifdef SA_AMD_DIAG
SA_EXPORT const char *sa_amd_version(void) { return "suffix_array_amd 0.2.0 (gfx950) DIAGNOSTIC BUILD"; }
#include "sa_diag.inc"
#else
SA_EXPORT const char *sa_amd_version(void) { return "suffix_array_amd 0.2.0 (gfx950)"; }
#endif

}  // extern "C"
