// host/support.hpp -- status mapping, launch checks, per-kernel event timing, small RAII helpers.
#pragma once
#include "../kernels/common.hpp"
#include "../kernels/keys.hpp"
#include "../kernels/radix_sort.hpp"
#include "../kernels/onesweep.hpp"
#include "../kernels/rerank.hpp"
#include "../kernels/refine.hpp"
#include "../kernels/bucket_sort.hpp"
#include "../kernels/isa.hpp"
#include "../kernels/extras.hpp"
#include "../kernels/small.hpp"
#ifdef SA_AMD_DIAG
#include "../kernels/sample_sort.hpp"
#include "../kernels/radix_sort_diag.hpp"
#include "../kernels/induce_proto.hpp"
#endif
#include "../../../include/suffix_array_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>
#include <chrono>
#include <sys/syscall.h>
#include <unistd.h>

namespace sa {

static inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static bool debug_sync()
{
    static int v = -1;
    if (v < 0) { const char *e = getenv("SA_AMD_DEBUG_SYNC"); v = (e && *e && *e != '0') ? 1 : 0; }
    return v == 1;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            if (getenv("SA_AMD_VERBOSE"))                                                          \
                fprintf(stderr, "suffix_array_amd: %s -> %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return e_ == hipErrorOutOfMemory ? SA_AMD_ENOMEM : SA_AMD_EHIP;                        \
        }                                                                                          \
    } while (0)

#define LAUNCH_CHECK(st)                                                                           \
    do {                                                                                           \
        HIP_TRY(hipGetLastError());                                                                \
        if (debug_sync()) HIP_TRY(hipStreamSynchronize(st));                                       \
    } while (0)

inline int hip_status(hipError_t e) { return e == hipSuccess ? SA_AMD_OK : (e == hipErrorOutOfMemory ? SA_AMD_ENOMEM : SA_AMD_EHIP); }

#ifdef SA_AMD_DIAG
// The fill switch of the diagnostic library only (sa_amd_debug_fill_blocks, csrc/sa_diag.h): while it is on,
// every pooled block, every zero-copy pinned block and every DevBuf is overwritten with the pattern before its first use, so
// that a route which reads a word it never wrote gives a wrong answer there instead of depending on its predecessor.
//   -1 off; 0 .. 255 that byte everywhere; 256 "small": word i = mix(i + seed) % 5; 257 "random": word i = mix(i + seed)
constexpr int FILL_OFF = -1, FILL_SMALL = 256, FILL_RANDOM = 257;
inline std::atomic<int> g_fill_pattern{FILL_OFF};
inline std::atomic<uint32_t> g_fill_seed{0};       // moves on with every fill: two blocks of a call do not hold the same words

__host__ __device__ static inline uint32_t fill_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ static inline uint32_t fill_word(uint32_t i, uint32_t seed, int pattern)
{
    const uint32_t m = fill_mix(i + seed);
    return pattern == FILL_SMALL ? m % 5u : m;
}

__global__ void __launch_bounds__(256) k_diag_fill(uint32_t *p, size_t words, uint32_t seed, int pattern)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) p[i] = fill_word((uint32_t)i, seed, pattern);
}

// `bytes` of device memory at `p` (4-byte aligned) on `st`, and a wait for it: whatever stream the route goes on to use, the
// fill is ordered before it.  The bytes behind the last whole word take the low byte of their word's pattern.
static inline int diag_fill_device(void *p, size_t bytes, hipStream_t st)
{
    const int pattern = g_fill_pattern.load(std::memory_order_relaxed);
    if (pattern == FILL_OFF || !p || bytes == 0) return SA_AMD_OK;
    hipError_t e = hipSuccess;
    if (pattern < FILL_SMALL) e = hipMemsetAsync(p, pattern, bytes, st);
    else {
        const uint32_t seed = g_fill_seed.fetch_add(0x9e3779b9u);
        const size_t words = bytes / 4, tail = bytes % 4;
        if (words > 0) {
            const size_t blocks = (words + 255) / 256;
            hipLaunchKernelGGL(k_diag_fill, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (uint32_t *)p, words, seed, pattern);
            e = hipGetLastError();
        }
        if (e == hipSuccess && tail > 0) e = hipMemsetAsync((char *)p + words * 4, (int)(fill_word((uint32_t)words, seed, pattern) & 0xffu), tail, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) (void)hipGetLastError();
    return hip_status(e);
}

// the same for a pinned host block that kernels reach zero-copy, written by the host before anything is queued on it
static inline void diag_fill_host(void *p, size_t bytes)
{
    const int pattern = g_fill_pattern.load(std::memory_order_relaxed);
    if (pattern == FILL_OFF || !p || bytes == 0) return;
    if (pattern < FILL_SMALL) { memset(p, pattern, bytes); return; }
    const uint32_t seed = g_fill_seed.fetch_add(0x9e3779b9u);
    const size_t words = bytes / 4;
    uint32_t *w = (uint32_t *)p;
    for (size_t i = 0; i < words; ++i) w[i] = fill_word((uint32_t)i, seed, pattern);
    for (size_t i = words * 4; i < bytes; ++i) ((uint8_t *)p)[i] = (uint8_t)fill_word((uint32_t)words, seed, pattern);
}

// The refusal switch and the ledger of the diagnostic library only (sa_amd_debug_refuse_alloc, sa_amd_debug_live_allocations,
// csrc/sa_diag.h; DESIGN.md section 10, "Refused allocations").  All memory the library takes goes through three seams --
// ResourcePool::acquire, ResourcePool::pinned (pool.hpp) and DevBuf::alloc (below) -- and each of them calls diag_request first,
// on the thread that called the seam: before the pool looks for a free block and before pinned() hands work to a helper, so
// that the count depends neither on what the pool holds nor on the thread that ends up calling the runtime.  A request that is
// to be refused asks the runtime for DIAG_REFUSED_BYTES, more than any device has: the runtime says no on the host, nobody's
// memory is taken, and the thread is left exactly as a real refusal leaves it (the runtime's per-thread error included).
enum { REQ_DEVICE = 1, REQ_PINNED = 2, REQ_TABLE = 3 };
constexpr size_t DIAG_REFUSED_BYTES = SIZE_MAX / 2;
constexpr int DIAG_KINDS_MAX = 64;
struct RefuseSwitch {
    int nth = -1;                 // -1 off (nothing is counted), 0 count only, k >= 1: the k-th request from arming on is refused, once
    int count = 0;                // requests since the switch was last set
    bool fired = false;
    uint8_t kinds[DIAG_KINDS_MAX] = { 0 };      // REQ_* of the first DIAG_KINDS_MAX counted requests
};
static thread_local RefuseSwitch g_refuse;
inline std::atomic<int64_t> g_live_device{0}, g_live_pinned{0};      // allocations made through the seams and not yet freed (process-wide)

// counts a request of `kind` of the calling thread; true: this one is to be refused
static inline bool diag_request(int kind)
{
    RefuseSwitch &r = g_refuse;
    if (r.nth < 0) return false;
    if (r.count < DIAG_KINDS_MAX) r.kinds[r.count] = (uint8_t)kind;
    ++r.count;
    if (r.nth >= 1 && r.count == r.nth && !r.fired) { r.fired = true; return true; }
    return false;
}
#define SA_DIAG_LIVE(counter, delta) ((void)sa::counter.fetch_add((delta), std::memory_order_relaxed))
#else
#define SA_DIAG_LIVE(counter, delta) ((void)0)
#endif

// device memory that is freed on every exit path (HIP_TRY returns early)
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf &operator=(DevBuf &&o) noexcept      // what this held is freed, what `o` held is this one's: `o` is left empty
    {
        if (this != &o) { reset(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // A refused allocation is SA_AMD_ENOMEM with nothing held, and the runtime's per-thread error is cleared here, once for every
    // caller: hipGetLastError keeps it until somebody reads it, and the next launch check of the thread would report it.
    int alloc(size_t bytes)
    {
        reset();
        size_t ask = bytes ? bytes : 1;
#ifdef SA_AMD_DIAG
        if (diag_request(REQ_TABLE)) ask = DIAG_REFUSED_BYTES;      // (sa_amd_debug_refuse_alloc: the runtime's own refusal, on the path below)
#endif
        const hipError_t e = hipMalloc(&p, ask);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return hip_status(e); }
        SA_DIAG_LIVE(g_live_device, 1);
        int rc = SA_AMD_OK;
#ifdef SA_AMD_DIAG
        rc = diag_fill_device(p, ask, nullptr);      // (an index's tables, the slack behind its text included)
#endif
        return rc;
    }
    void reset() { if (p) { (void)hipFree(p); SA_DIAG_LIVE(g_live_device, -1); } p = nullptr; }
    template <typename T> T *as() const { return (T *)p; }
};

// the number of HIP devices (0 where the runtime cannot tell): what sa_amd_device_count answers
static inline int device_count()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    return ndev;
}

// makes `device` current for the scope and restores the caller's device afterwards (device < 0: leave it alone)
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int rc = SA_AMD_OK;
    explicit DeviceGuard(int device)
    {
        if (device < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) { rc = SA_AMD_EHIP; return; }
        if (prev != device) { rc = hip_status(hipSetDevice(device)); switched = rc == SA_AMD_OK; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// the body of every extern "C" entry point runs inside this: nothing may unwind through the C ABI
#define SA_ABI_GUARD_BEGIN try {
#define SA_ABI_GUARD_END(fallback)                                                                 \
    } catch (const std::bad_alloc &) { return (fallback) == 0 ? SA_AMD_ENOMEM : (fallback); }      \
      catch (...) { return (fallback) == 0 ? SA_AMD_EINTERNAL : (fallback); }

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// the grid of a kernel whose blocks stride over their work: one block per `per_block` items, `cap` blocks at the most
static inline unsigned capped_grid(int64_t items, int64_t per_block, int64_t cap) { const int64_t b = ceil_div(items, per_block); return (unsigned)(b < cap ? b : cap); }
static inline int bit_length(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- optional per-kernel timing with HIP events on the launch stream (bench.py roofline) ----
enum KClass { KC_BYTE_HIST = 0, KC_BUILD_KEYS, KC_UPSWEEP, KC_SPINE, KC_DOWNSWEEP, KC_RR_COUNT, KC_RR_SCAN, KC_RR_APPLY,
              KC_GATHER, KC_SCATTER, KC_LOCAL, KC_MISC, KC_UPSWEEP32, KC_DOWNSWEEP32, KC_ONESWEEP, KC_ONESWEEP32, KC_FINISH, KC_BUCKET,
              KC_LCP_PHI, KC_LCP_IRRED, KC_LCP_LONG, KC_LCP_SCAN, KC_LCP_GATHER,
              KC_BWT_GATHER, KC_UNBWT_WALK, KC_UNBWT_RANK, KC_UNBWT_WRITE,
#ifdef SA_AMD_DIAG
              KC_SS_COUNT, KC_SS_SCATTER, KC_SS_BUCKET,
#endif
              KC_REP_LR, KC_REP_SPANS,         // (behind every earlier class of either library: no index moves)
              KC_COUNT };
static_assert(KC_COUNT <= 32, "bench.py reads 32 kernel classes");
static const char *const kclass_names[KC_COUNT] = { "k_byte_hist", "k_build_keys", "k_radix_upsweep", "k_spine_rows",
                                                    "k_radix_downsweep", "k_rr_count", "k_rr_scan", "k_rr_apply",
                                                    "k_gather_key2", "k_scatter_pairs", "k_group_sort", "misc",   // (k_gather_key2: the plain gathers; k_group_sort: all fused gather + sort kernels)
                                                    "k_radix_upsweep32", "k_radix_downsweep32",
                                                    "k_onesweep", "k_onesweep32",      // single-pass tile scatter, 64- / 32-bit keys (kernels/onesweep.hpp)
                                                    "k_finish_sorted",                 // one pass over the sorted keys that orders the small groups in place
                                                    "k_bucket_sort",                   // the low 16 bits of the 32-bit first stage, bucket by bucket in LDS (kernels/bucket_sort.hpp)
                                                    "k_lcp_phi", "k_lcp_irreducible",  // LCP array (kernels/lcp.hpp): range pass + plain Φ scatter, irreducible values up to the cap,
                                                    "k_lcp_long", "k_lcp_scan",        // long compares + settle, max-scan (spine + tiles),
                                                    "k_lcp_gather",                    // LCP[i] = PLCP[SA[i]]
                                                    "k_bwt_gather", "k_unbwt_walk",    // Burrows-Wheeler transform (kernels/bwt.hpp): range pass + gather; inverse: splitters + walks,
                                                    "k_unbwt_rank", "k_unbwt_write"    // pointer jumping over the sublists, second walk that writes the text
#ifdef SA_AMD_DIAG
                                                    , "k_ss_count", "k_ss_scatter",    // diagnostic library: sample sort of the 64-bit stage (kernels/sample_sort.hpp), the two distribution
                                                    "k_ss_bucket_sort"                 // levels and every bucket ordered in LDS
#endif
                                                    , "k_rep_lr", "k_rep_spans"        // repeat finder (kernels/repeats.hpp): slot pass + KEEP_FIRST flags, the span passes
                                                    };
struct Profiler {
    bool on = false;
    uint64_t mask = ~0ull;      // kernel classes that get events (each pair costs a few microseconds of host time)
    struct Rec { int cls; hipEvent_t a, b; int64_t units; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    double ms[KC_COUNT] = { 0 };
    int64_t launches[KC_COUNT] = { 0 }, units[KC_COUNT] = { 0 };
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void begin(int cls, int64_t u, hipStream_t st)
    {
        open = on && ((mask >> cls) & 1ull);
        if (!open) return;
        Rec r; r.cls = cls; r.units = u; r.a = get(); r.b = get();
        (void)hipEventRecord(r.a, st);
        recs.push_back(r);
    }
    bool open = false;
    void end(hipStream_t st) { if (open && !recs.empty()) (void)hipEventRecord(recs.back().b, st); open = false; }
    ~Profiler()      // (a worker thread of sa_amd_saca_batch that profiled must not leak its events)
    {
        if ((long)syscall(SYS_gettid) == (long)getpid()) return;      // the main thread's copy dies at process exit: no HIP calls then
        for (auto &r : recs) { if (r.a) (void)hipEventDestroy(r.a); if (r.b) (void)hipEventDestroy(r.b); }
        for (auto e : pool) if (e) (void)hipEventDestroy(e);
    }
    void resolve()   // call after the stream has been synchronised
    {
        for (auto &r : recs) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms[r.cls] += t; launches[r.cls]++; units[r.cls] += r.units; }
            pool.push_back(r.a); pool.push_back(r.b);
        }
        recs.clear();
    }
};
static thread_local Profiler g_prof;
static thread_local sa_amd_stats g_last_stats;
#define PROF(cls, units, st, launch_stmt)                                                          \
    do { g_prof.begin(cls, units, st); launch_stmt; g_prof.end(st); LAUNCH_CHECK(st); } while (0)

}  // namespace sa
