// host/extras.hpp -- the routes of kernels/extras.hpp and the device-resident index's own: bucket table and integrity check
// (device pointers, host buffers, an index), creation of an index, the packed format.
#pragma once
#include "scope.hpp"
#include "index.hpp"

namespace sa {

// ---- bucket table and integrity check on device-resident arrays ----

// dBkt: BKT_LEN entries.  With dSA one binary search per bucket edge, without it the text's bigram counts.  Blocks until done.
static int32_t bucket_table_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dBkt, hipStream_t st)
{
    if (n < 0 || !dBkt || (n > 0 && !dT)) return SA_AMD_EINVAL;
    if (dSA) {
        // a device-resident index has the sorted order at hand: one binary search per bucket edge (~0.08 ms whatever n)
        hipLaunchKernelGGL(k_bucket_table, dim3((BKT_LEN + 255) / 256), dim3(256), 0, st, dT, dSA, (int64_t)n, dBkt);
    } else {
        // as the reference builds it (src/sa.rs:96-116): bigram counts of the text + prefix sum, no suffix array needed.  The
        // counts live in the first 65 536 words of dBkt itself (k_bigram_scan reads them all before it writes)
        if (hipMemsetAsync(dBkt, 0, (size_t)65536 * 4, st) != hipSuccess) return SA_AMD_EHIP;
        int64_t pairs = ceil_div((int64_t)n, BG_MIN_CHUNK);
        if (pairs > BG_MAX_PAIRS) pairs = BG_MAX_PAIRS;
        if (n >= 2)
            hipLaunchKernelGGL(k_bigram_hist, dim3((unsigned)(2 * pairs)), dim3(BG_THREADS), 0, st, dT, (int64_t)n, (int)pairs, dBkt);
        hipLaunchKernelGGL(k_bigram_scan, dim3(1), dim3(BGS_THREADS), 0, st, (const uint32_t *)dBkt, dT, (int64_t)n, dBkt);
    }
    if (hipGetLastError() != hipSuccess) return SA_AMD_EHIP;
    return hipStreamSynchronize(st) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

// layout of the larger work block (fast form): flags | rank | four pair buffers | spine + digit totals | granules + error word
struct CiLayout { size_t flags, rank, alt, alt_elems, spine, status, err, starts, bitmap, bitmap_bytes, bytes; };
static CiLayout ci_layout(int32_t n)
{
    CiLayout L;
    const size_t N1 = (size_t)n + 1;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = align_up(off + b, 256); return o; };
    L.flags = take(256);
    L.rank = take(N1 * 4);
    L.alt_elems = (N1 + 67) & ~(size_t)3;
    L.alt = take(4 * L.alt_elems * 4);
    L.spine = take(SortScratch::SPINE_BYTES);
    L.status = take(SortScratch::granule_bytes((int64_t)N1));
    L.err = take(256);
    L.starts = take(257 * 4);
    L.bitmap_bytes = ((N1 + 31) / 32 + 1) * 4;
    L.bitmap = take(L.bitmap_bytes);
    L.bytes = off;
    return L;
}

// dWork: at least 4 (n + 1) + 256 bytes (the small form), ci_layout(n).bytes and 256-byte aligned for the streaming form;
// arguments checked by the caller.  1: a suffix array, 0: not one, or an error code.  Blocks until done.
static int32_t check_integrity_device(const uint8_t *dT, int32_t n, const uint32_t *dSA, void *dWork, int64_t work_bytes, hipStream_t st)
{
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
        uint32_t *rank_of = (uint32_t *)(base + L.rank);
        const SortScratch ss = SortScratch::make(base + L.spine, base + L.status, (uint32_t *)(base + L.err));
        HIP_TRY(hipMemsetAsync(ss.err, 0, 16, st));
        uint32_t *alt = (uint32_t *)(base + L.alt);
        const Tuning tn = env_tuning();
        sa_amd_stats local;
        memset(&local, 0, sizeof(local));
        // pairs (SA[i], i), i = 0 .. n, binned by the suffix position; the scatter skips the empty suffix (value n)
        const int rcs = scatter_binned(ss, rank_of, (uint32_t *)dSA, nullptr, alt, alt + L.alt_elems, (int64_t)n + 1, (int64_t)n, st, &local, tn, true,
                                       alt + 2 * L.alt_elems, alt + 3 * L.alt_elems);
        if (rcs) return rcs;
        // first bytes: boundaries proposed from the array, proved in text order (streaming); then the slot-order check
        uint32_t *starts = (uint32_t *)(base + L.starts), *bitmap = (uint32_t *)(base + L.bitmap);
        HIP_TRY(hipMemsetAsync(bitmap, 0, L.bitmap_bytes, st));
        hipLaunchKernelGGL(k_ci_starts, dim3(1), dim3(512), 0, st, dT, dSA, (int64_t)n, starts, bitmap);
        int64_t fblocks = ceil_div((int64_t)n, 256 * 16);
        if (fblocks > 16384) fblocks = 16384;
        hipLaunchKernelGGL(k_ci_first_bytes, dim3((unsigned)fblocks), dim3(256), 0, st, dT, (int64_t)n, (const uint32_t *)rank_of, (const uint32_t *)starts, flags);
        const int64_t cblocks = ceil_div((int64_t)n, (int64_t)CI_THREADS * CI_ITEMS);
        hipLaunchKernelGGL(k_ci_check_shared, dim3((unsigned)cblocks), dim3(CI_THREADS), 0, st, dSA, (int64_t)n, (const uint32_t *)rank_of,
                           (const uint32_t *)bitmap, flags);
        HIP_TRY(hipGetLastError());
        uint32_t words[2] = { 0, 0 };
        { const int rcw = read_words(&words[0], flags, 4, st); if (rcw) return rcw; }
        { const int rcw = read_words(&words[1], ss.err, 4, st); if (rcw) return rcw; }
        if (words[1]) return SA_AMD_EINTERNAL;
        return (words[0] & 2u) ? 0 : 1;
    }
    // ---- small work block (4 (n + 1) + 256 bytes): random-store inverse, three rank reads per slot ----
    hipLaunchKernelGGL(k_ci_scatter, dim3((unsigned)blocks), dim3(256), 0, st, dSA, (int64_t)n, rank, flags);
    hipLaunchKernelGGL(k_ci_check, dim3((unsigned)blocks), dim3(256), 0, st, dT, dSA, (int64_t)n, (const uint32_t *)rank, flags);
    if (hipGetLastError() != hipSuccess) return SA_AMD_EHIP;
    uint32_t f = 0;
    if (hipMemcpyAsync(&f, flags, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return SA_AMD_EHIP;
    if (hipStreamSynchronize(st) != hipSuccess) return SA_AMD_EHIP;
    if (f & 1u) return SA_AMD_ERANGE;
    return (f & 2u) ? 0 : 1;
}

// enable_buckets on host buffers (reference src/sa.rs:89-119): the text goes up, 257 KiB come back; nothing else is needed --
// the reference builds the table from the text alone.
static int32_t bucket_table_host(const uint8_t *T, int32_t n, uint32_t *bkt)
{
    if (n < 0 || !bkt || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
    const size_t tb = align_up((size_t)n + 16, 256);
    PooledScope sc(pick_device(), true);
    sc.acquire(tb + (size_t)BKT_LEN * 4);
    uint8_t *dT = (uint8_t *)sc.take(tb);
    uint32_t *dB = (uint32_t *)sc.take((size_t)BKT_LEN * 4);
    if (sc.rc == SA_AMD_OK && n > 0) sc.rc = hip_status(hipMemcpyAsync(dT, T, (size_t)n, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK) sc.rc = bucket_table_device(dT, nullptr, n, dB, sc.st);
    sc.down(bkt, dB, (size_t)BKT_LEN * 4);
    return sc.finish();
}

// host buffers; which = 2: integrity check, 3: build SA (into SA, n + 1 entries) then bucket table
static int32_t extras_host(const uint8_t *T, int32_t n, uint32_t *SA, int64_t sa_len, uint32_t *bkt, int which)
{
    if (n < 0 || !SA || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
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
        const int64_t wb = (int64_t)carve(nullptr, n).bytes;
        // every buffer is taken, and both results exist on the device, before either comes down: outputs are written only
        // after the last step that can fail
        if ((rc = dW.alloc((size_t)wb))) return rc;
        if ((rc = dB.alloc((size_t)BKT_LEN * 4))) return rc;
        if ((rc = build_device(dT.as<uint8_t>(), dSA.as<uint32_t>(), n, dW.p, wb, nullptr, nullptr))) return rc;
        // the text is in HBM already: the table from its bigrams, as the reference counts them
        if ((rc = bucket_table_device(dT.as<uint8_t>(), nullptr, n, dB.as<uint32_t>(), nullptr))) return rc;
        HIP_TRY(hipMemcpy(SA, dSA.p, (N + 1) * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(bkt, dB.p, (size_t)BKT_LEN * 4, hipMemcpyDeviceToHost));
        return SA_AMD_OK;
    }
    HIP_TRY(hipMemcpy(dSA.p, SA, (N + 1) * 4, hipMemcpyHostToDevice));
    int64_t wb = (int64_t)ci_layout(n).bytes;              // the streaming form; the small block if that much is not to be had
    rc = dW.alloc((size_t)wb);
    if (rc == SA_AMD_ENOMEM) { wb = ((int64_t)n + 1) * 4 + 256; rc = dW.alloc((size_t)wb); }
    if (rc) return rc;
    return check_integrity_device(dT.as<uint8_t>(), n, dSA.as<uint32_t>(), dW.p, wb, nullptr);
}

// ---- the device-resident index: creation, its array, bucket table and integrity check ----

// sa_amd_index_create behind its argument checks: the text goes up, and the caller's array (SA, n + 1 entries) or, SA == nullptr,
// the one built on the device (SuffixArray::new); *out owns both
static int32_t index_create(const uint8_t *T, int32_t n, const uint32_t *SA, sa_amd_index **out)
{
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
        const int64_t wb = (int64_t)carve(nullptr, n).bytes;
        if ((rc = dW.alloc((size_t)wb))) return rc;
        if ((rc = build_device(dT.as<uint8_t>(), dSA.as<uint32_t>(), n, dW.p, wb, nullptr, nullptr))) return rc;
    }
    sa_amd_index *ix = new (std::nothrow) sa_amd_index();
    if (!ix) return SA_AMD_ENOMEM;
    ix->n = n;
    (void)hipGetDevice(&ix->device);
    ix->dT = std::move(dT);
    ix->dSA = std::move(dSA);
    *out = ix;
    return SA_AMD_OK;
}

static int32_t index_sa(const sa_amd_index &ix, uint32_t *SA_out)
{
    DeviceGuard guard(ix.device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return hipMemcpy(SA_out, ix.sa(), ((size_t)ix.n + 1) * 4, hipMemcpyDeviceToHost) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

// the table is built by the first call and kept: later searches start from the pattern's bucket
static int32_t index_buckets(sa_amd_index &ix, uint32_t *bkt)
{
    PooledScope sc(ix.device, false);                           // (no block: the build needs none)
    if (sc.rc) return sc.rc;
    if (!ix.bkt()) {
        DevBuf dB;
        if (index_table_alloc(dB, (size_t)BKT_LEN * 4) != SA_AMD_OK) return SA_AMD_ENOMEM;
        sc.rc = bucket_table_device(ix.text(), ix.sa(), ix.n, dB.as<uint32_t>(), sc.st);
        if (sc.finish() != SA_AMD_OK) return sc.rc;
        ix.dBkt = std::move(dB);
    }
    return hipMemcpy(bkt, ix.bkt(), (size_t)BKT_LEN * 4, hipMemcpyDeviceToHost) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

// 1 / 0, or a code
static int32_t index_check_integrity(const sa_amd_index &ix)
{
    // the work block of the streaming form comes from the process-wide pool (a 5.5 GB hipMalloc / hipFree per call would
    // cost more than the check); the small block if that much is not to be had
    PooledScope sc(ix.device, false);
    int64_t wb = (int64_t)ci_layout(ix.n).bytes;
    if (sc.acquire((size_t)wb) == SA_AMD_ENOMEM) { wb = ((int64_t)ix.n + 1) * 4 + 256; sc.acquire_smaller((size_t)wb); }
    if (sc.rc) return sc.rc;
    const int32_t ok = check_integrity_device(ix.text(), ix.n, ix.sa(), sc.take((size_t)wb), wb, nullptr);
    if (ok < 0) sc.rc = ok;
    (void)sc.finish();
    return ok;
}

// ---- packed format (reference src/packed_sa.rs); byte layout: u32 magic "SA4x" LE, u32 length, u64 data length
//      (bincode's Vec<u8> prefix), data ----

static int sa_bits_of(uint32_t length)          // reference src/packed_sa.rs:127-129
{
    const uint32_t v = length ? length - 1 : 0;
    return v ? bit_length(v) : 0;
}

// length in 0 .. 2^32 - 1
static int64_t pack_bound(int64_t length)
{
    const int bits = sa_bits_of((uint32_t)length);
    return 16 + (int64_t)((length + 127) / 128) * bits * 16;
}

static int32_t pack(const uint32_t *SA, int64_t length, uint8_t *out, int64_t capacity, int64_t *out_len)
{
    if (!SA || !out || !out_len || length < 1 || length > 0xffffffffLL) return SA_AMD_EINVAL;
    if (capacity < pack_bound(length)) return SA_AMD_EINVAL;
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
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
}

static int32_t unpack(const uint8_t *bytes, int64_t nbytes, uint32_t *SA, int64_t capacity, int64_t *length)
{
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
    if (device_count() <= 0) return SA_AMD_ENODEVICE;
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
}

}  // namespace sa
