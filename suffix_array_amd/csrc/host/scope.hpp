// host/scope.hpp -- what every route that works in a pooled device block shares ("Pooled-block scope"):
//   PooledScope    the route's device, stream and block, given back on every path out; the route's return code
//   upload_inputs  text up, then the caller's suffix array up or build_device into the block (resident_inputs: an index's)
//   CappedRows     "the first `cap` rows, the count of all rows" outputs (repeat spans, LZ77 phrases, match spans)
// New routes use these; nothing outside this file, pool.hpp and host_path.hpp calls the pool's acquire / release by hand.
#pragma once
#include "pipeline.hpp"
#include "host_path.hpp"

namespace sa {

// Makes `device` current (< 0: the caller's stays), optionally takes a pooled stream (else the null stream), and holds one pooled
// block that take() carves into 256-byte aligned slabs.  rc is the route's return code: the first failure, from opening
// onwards; every step of a route runs only while it is SA_AMD_OK.  On the way out the stream is drained BEFORE the block goes
// back to the pool, then the stream goes back, then the caller's device is restored -- after finish(), after an early return,
// and when an exception is on its way to the ABI guard.  A route on the null stream that succeeded has nothing queued (the
// *_device calls block, down() is hipMemcpy there): finish() waits on the null stream only after a failure.
struct PooledScope {
    DeviceGuard guard;
    int device = 0;
    PooledStream ps{-1};
    DevBlock blk;
    size_t need = 0, used = 0;      // bytes asked of the pool; bytes handed out by take()
    hipStream_t st = nullptr;       // ps.st, or the null stream
    bool drained = false;
    int32_t rc;

    PooledScope(int dev, bool pooled_stream) : guard(dev), rc(guard.rc)
    {
        if (rc == SA_AMD_OK && hipGetDevice(&device) != hipSuccess) rc = SA_AMD_EHIP;
        if (rc == SA_AMD_OK && pooled_stream) { ps.device = device; rc = pool().stream(device, &ps.st); st = ps.st; }
    }
    PooledScope(const PooledScope &) = delete;
    PooledScope &operator=(const PooledScope &) = delete;
    ~PooledScope()
    {
        if (!blk.p) return;
        if (!drained) (void)hipStreamSynchronize(st);
        pool().release(blk);
    }
    // exactly `bytes` are asked of the pool (its retention policy keys on the sizes).  Once per scope, unless it failed.
    int32_t acquire(size_t bytes)
    {
        if (rc == SA_AMD_OK) { need = bytes; rc = pool().acquire(device, bytes, &blk); }
#ifdef SA_AMD_DIAG
        if (rc == SA_AMD_OK) rc = diag_fill_device(blk.p, need, st);      // (sa_amd_debug_fill_blocks: the bytes asked for, before the first slab is used)
#endif
        return rc;
    }
    // a smaller block where acquire() answered SA_AMD_ENOMEM (nothing is held then); any other state stays as it is
    int32_t acquire_smaller(size_t bytes)
    {
        if (rc == SA_AMD_ENOMEM && !blk.p) { rc = SA_AMD_OK; return acquire(bytes); }
        return rc;
    }
    // the next slab.  The first one starts the block: the only address known to be 256-byte aligned, so the work block goes
    // first.  nullptr on a scope that failed; a slab that ends behind the bytes acquired is SA_AMD_EINTERNAL.
    void *take(size_t bytes)
    {
        if (rc != SA_AMD_OK) return nullptr;
        if (used + bytes > need) { rc = SA_AMD_EINTERNAL; return nullptr; }
        void *p = (char *)blk.p + used;
        used += align_up(bytes, 256);
        return p;
    }
    // device -> caller's buffer: behind the work on the pooled stream, or hipMemcpy on the null stream (as the index routes
    // always copied)
    void down(void *dst, const void *src, size_t bytes)
    {
        if (rc != SA_AMD_OK) return;
        rc = hip_status(ps.st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    }
    // the end of every route: waits for the stream (a pooled one always; the null stream after a failure) and returns the
    // first failure, else the wait's code
    int32_t finish()
    {
        if (blk.p && !drained && (ps.st || rc != SA_AMD_OK)) {
            const int32_t rs = hip_status(hipStreamSynchronize(st));
            if (rc == SA_AMD_OK) rc = rs;
        }
        drained = true;
        return rc;
    }
};

// The resident inputs of a route: work block | text | suffix array, in this order at the start of the scope's block.
struct Inputs { void *dW = nullptr; const uint8_t *dT = nullptr; const uint32_t *dSA = nullptr; size_t wb = 0; };

// Acquires work block + text + array + `out_bytes` (the caller's output slabs, each rounded up to 256), sends the text up and
// then the caller's array (n + 1 entries) -- or, SA == nullptr, builds the array in the block, for which the work block is at
// least the construction's.  n == 0: no text travels, the one-entry array still does.
static Inputs upload_inputs(PooledScope &sc, const uint8_t *T, int32_t n, const uint32_t *SA, size_t layout_bytes, size_t out_bytes)
{
    const size_t N1 = (size_t)n + 1;
    Inputs in;
    in.wb = layout_bytes;
    if (!SA) { const size_t bb = (size_t)carve(nullptr, n).bytes; in.wb = bb > in.wb ? bb : in.wb; }
    sc.acquire(in.wb + align_up((size_t)n + 16, 256) + align_up(N1 * 4, 256) + out_bytes);
    in.dW = sc.take(in.wb);
    uint8_t *dT = (uint8_t *)sc.take((size_t)n + 16);
    uint32_t *dSA = (uint32_t *)sc.take(N1 * 4);
    in.dT = dT; in.dSA = dSA;
    if (sc.rc == SA_AMD_OK && n > 0) sc.rc = hip_status(hipMemcpyAsync(dT, T, (size_t)n, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK)
        sc.rc = SA ? hip_status(hipMemcpyAsync(dSA, SA, N1 * 4, hipMemcpyHostToDevice, sc.st)) : build_device(dT, dSA, n, in.dW, (int64_t)in.wb, sc.st, nullptr);
    return in;
}

// The same for a text and array that are resident already (a device index): work block + exactly `out_bytes` (the sum the
// index routes have always asked for: their last output slab is not rounded up).
static Inputs resident_inputs(PooledScope &sc, const uint8_t *dT, const uint32_t *dSA, size_t work_bytes, size_t out_bytes)
{
    Inputs in;
    in.dT = dT; in.dSA = dSA; in.wb = work_bytes;
    sc.acquire(work_bytes + out_bytes);
    in.dW = sc.take(work_bytes);
    return in;
}

// Rows of 8 bytes of which the caller takes the first `capacity` and learns the number of all: no more than the feature's
// bound can exist, whatever the caller's capacity, so the slab holds min(capacity, bound) rows (+ 8 bytes: never empty).
struct CappedRows {
    int64_t cap = 0, count = 0;
    CappedRows() = default;
    CappedRows(int64_t capacity, int64_t bound) : cap(capacity < bound ? capacity : bound) {}
    size_t bytes() const { return (size_t)cap * 8 + 8; }
    // the end of a route whose device call left `count`: min(count, cap) rows come down, and only when all of the route
    // succeeded, after the wait, is *count_out written
    int32_t finish(PooledScope &sc, uint32_t *out, const uint32_t *dRows, int64_t *count_out) const
    {
        const int64_t wr = count < cap ? count : cap;
        if (wr > 0) sc.down(out, dRows, (size_t)wr * 8);
        if (sc.finish() == SA_AMD_OK) *count_out = count;
        return sc.rc;
    }
};

}  // namespace sa
