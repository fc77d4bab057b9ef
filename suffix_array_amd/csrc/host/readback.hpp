// host/readback.hpp -- small device -> host read-backs of the device pipeline (host/pipeline.hpp, host/refine_round.hpp): read_words.
#pragma once
#include "support.hpp"
#include "pool.hpp"

namespace sa {

// Small device -> host read-backs (counts that steer the host loop) go through a pinned per-thread buffer:
// a 4-byte hipMemcpyAsync into pageable memory costs ~50-90 us per round trip, into pinned memory ~10.
// The buffer is a block of the process-wide pool: a short-lived worker thread (sa_amd_saca_batch) hands it back when it
// exits instead of paying hipHostMalloc / hipHostFree per call; a failed allocation is remembered, not retried per call.
struct PinnedWords {
    PinBlock b;
    bool failed = false;
    ~PinnedWords() { if (b.p) pool().release_pinned(b); }
};
static thread_local PinnedWords g_pinned;
static thread_local int g_readbacks = 0;        // blocking read-backs of the calling thread's current build (sa_amd_stats.readbacks)
static thread_local bool g_posted_off = false;  // SA_AMD_NO_POSTED_READBACK (set per build from the tuning)
// tags of posted read-backs: process-wide, so a block another thread used before cannot hold the tag this thread waits for
static std::atomic<uint32_t> g_post_seq{0};

// A read-back as a POSTED write: one tiny kernel stores the words into the (mapped) pinned block, every 64-byte line tagged with
// a sequence number, and the host spins on the tags -- instead of a copy command plus hipStreamSynchronize, whose wake-up costs
// more than the kernel (measured, tools/readback_probe.hip: kernel + copy + synchronise 15.0 us, kernel + post kernel + spin
// 10.2 us, kernel + synchronise alone 11.4 us).  Line q of the block = [tag, words 15q .. 15q + 14]; the tag sits in the same
// line as the data it vouches for, so a line is either old or complete whatever the order the lines arrive in.
constexpr int POST_LINE = 16;
__global__ __launch_bounds__(256) void k_post_words(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int words, uint32_t seq)
{
    const int lines = (words + POST_LINE - 2) / (POST_LINE - 1);
    for (int i = threadIdx.x; i < lines * POST_LINE; i += 256) {
        const int q = i / POST_LINE, j = i % POST_LINE;
        if (j) { const int k = q * (POST_LINE - 1) + j - 1; dst[i] = k < words ? src[k] : 0u; }
    }
    __threadfence_system();
    __syncthreads();
    for (int q = threadIdx.x; q < lines; q += 256) __hip_atomic_store(dst + q * POST_LINE, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The thread's block is 8 KiB: the tagged lines of the posted path in the lower half (zeroed when the block is taken: a recycled
// block holds old tags), the plain copy in the upper half (raw words, no tags).
static int read_words(void *dst, const void *dsrc, size_t bytes, hipStream_t st)     // bytes <= 3840, a multiple of 4; synchronises the stream
{
    ++g_readbacks;
    if (!g_pinned.b.p && !g_pinned.failed) {
        if (pool().pinned(8192, -1, -1, &g_pinned.b) == SA_AMD_OK) memset(g_pinned.b.p, 0, 8192);
        else g_pinned.failed = true;
    }
    if (!g_pinned.b.p) {
        HIP_TRY(hipMemcpyAsync(dst, dsrc, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SA_AMD_OK;
    }
    const int words = (int)(bytes / 4);
    const int lines = (words + POST_LINE - 2) / (POST_LINE - 1);
    if (!g_posted_off && (bytes & 3) == 0 && words > 0 && (size_t)lines * POST_LINE * 4 <= 4096) {
        uint32_t *host = (uint32_t *)g_pinned.b.p;
        uint32_t seq = g_post_seq.fetch_add(1, std::memory_order_relaxed) + 1;
        if (seq == 0) seq = g_post_seq.fetch_add(1, std::memory_order_relaxed) + 1;      // (0 is what a fresh block holds)
        // (the pool's pinned blocks are portable and mapped: the host address is valid on every device)
        hipLaunchKernelGGL(k_post_words, dim3(1), dim3(256), 0, st, (const uint32_t *)dsrc, host, words, seq);
        if (hipGetLastError() == hipSuccess) {
            const auto t0 = std::chrono::steady_clock::now();
            bool done = false, finished = false;
            for (unsigned spin = 0; !done; ++spin) {
                done = true;
                for (int q = lines - 1; q >= 0 && done; --q)
                    done = __atomic_load_n((volatile uint32_t *)(host + q * POST_LINE), __ATOMIC_ACQUIRE) == seq;
                if (done) break;
                if ((spin & 1023u) == 1023u) {
                    // the stream has drained and the tags are still not there (a second look after the query): the copy path decides
                    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
                    if (us > 200.0) {
                        if (finished) break;
                        const hipError_t q = hipStreamQuery(st);
                        if (q == hipSuccess) finished = true;
                        else if (q != hipErrorNotReady) { (void)hipGetLastError(); break; }
                    }
                }
            }
            if (done) {
                uint32_t *out = (uint32_t *)dst;
                for (int k = 0; k < words; ++k) out[k] = host[(k / (POST_LINE - 1)) * POST_LINE + 1 + k % (POST_LINE - 1)];
                return SA_AMD_OK;
            }
        }
    }
    char *copy = (char *)g_pinned.b.p + 4096;
    HIP_TRY(hipMemcpyAsync(copy, dsrc, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(dst, copy, bytes);
    return SA_AMD_OK;
}

}  // namespace sa
