// sa_api.hip -- the C ABI (include/suffix_array_amd.h) of the MI355X-native suffix-array construction engine.
// Replaces the body of `saca()` (reference src/saca.rs:9-15) and the C engine behind
// `cdivsufsort::sort_in_place` (src/saca.rs:14).
//
// This file is the ABI layer only: per entry point the argument checks, the guard and ONE call into namespace sa; the bodies
// live next to their kernels' host code in host/*.hpp (the device-resident index itself: host/index.hpp), and no entry point
// launches, allocates, copies or calls another entry point.
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
#include "host/index.hpp"
#include "host/extras.hpp"
#include "host/lcp.hpp"
#include "host/esa.hpp"
#include "host/bwt.hpp"
#include "host/repeats.hpp"
#include "host/lz.hpp"
#include "host/match.hpp"
#include "host/docs.hpp"
#include "host/doc_match.hpp"
#include "host/doc_repeats.hpp"
#include "host/doc_tf.hpp"
#include "host/substrings.hpp"
#include "host/doc_substrings.hpp"
#include "host/ngram.hpp"
#include "host/score.hpp"
#include "host/tokens.hpp"

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
    return sa::saca_batch(T, SA, n, device, count, status, ndev);
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
    return sa::bucket_table_device(dT, dSA, n, dBkt, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int64_t sa_amd_check_integrity_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::ci_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_check_integrity_device(const uint8_t *dT, int32_t n, const uint32_t *dSA, void *dWork,
                                                int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || (n > 0 && !dT)) return SA_AMD_EINVAL;
    if (work_bytes < ((int64_t)n + 1) * 4 + 256) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::check_integrity_device(dT, n, dSA, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_bucket_table(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *bkt)
{
    if (!bkt) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    (void)SA;                       // (the reference builds the table from the text alone, src/sa.rs:96-116)
    return sa::bucket_table_host(T, n, bkt);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_saca_u8_buckets(const uint8_t *T, uint32_t *SA, int32_t n, uint32_t *bkt)
{
    if (!bkt) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::extras_host(T, n, SA, (int64_t)n + 1, bkt, 3);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_check_integrity(const uint8_t *T, int32_t n, const uint32_t *SA, int64_t sa_len)
{
    SA_ABI_GUARD_BEGIN
    return sa::extras_host(T, n, (uint32_t *)SA, sa_len, nullptr, 2);
    SA_ABI_GUARD_END(0)
}

// ---- device-resident index (host/index.hpp): text + suffix array kept in HBM for bucket table, integrity check and batched search ----

SA_EXPORT int32_t sa_amd_index_create(const uint8_t *T, int32_t n, const uint32_t *SA, sa_amd_index **out)
{
    if (!out || n < 0 || (n > 0 && !T)) return SA_AMD_EINVAL;
    *out = nullptr;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    return sa::index_create(T, n, SA, out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_index_destroy(sa_amd_index *ix)      // (frees and deletes: nothing that throws, no change of device)
{
    delete ix;
}

SA_EXPORT int32_t sa_amd_index_sa(const sa_amd_index *ix, uint32_t *SA_out)
{
    if (!ix || !SA_out) return SA_AMD_EINVAL;
    return sa::index_sa(*ix, SA_out);
}

SA_EXPORT int32_t sa_amd_index_buckets(sa_amd_index *ix, uint32_t *bkt)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !bkt) return SA_AMD_EINVAL;
    return sa::index_buckets(*ix, bkt);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_check_integrity(const sa_amd_index *ix)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::index_check_integrity(*ix);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_search(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count,
                                      uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi, uint32_t *lcp_start,
                                      uint32_t *lcp_len)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count)) return SA_AMD_EINVAL;
    return sa::index_search(*ix, pat_data, pat_off, count, contains, range_lo, range_hi, lcp_start, lcp_len);
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
    return sa::lcp_index(*ix, LCP);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_enable_lcp(sa_amd_index *ix)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::index_enable_lcp(*ix);
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
    return sa::bwt_index(*ix, BWT, primary_out);
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

SA_EXPORT int32_t sa_amd_index_repeat_lengths(const sa_amd_index *ix, uint32_t *LR)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::repeats_index(*ix, false, LR, 1, 0, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_repeat_spans(const sa_amd_index *ix, int32_t min_len, int32_t mode, uint32_t *spans, int64_t capacity,
                                            int64_t *count_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::repeats_index(*ix, true, nullptr, min_len, mode, spans, capacity, count_out);
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

SA_EXPORT int32_t sa_amd_index_lpf(const sa_amd_index *ix, uint32_t *LPF, uint32_t *SRC)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::lz_index(*ix, false, LPF, SRC, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_lz77(const sa_amd_index *ix, uint32_t *phrases, int64_t capacity, int64_t *count_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::lz_index(*ix, true, nullptr, nullptr, phrases, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_lz_stats(sa_amd_lz_stats *out)
{
    if (out) *out = sa::g_last_lz_stats;
}

// ---- matching statistics and shared spans of a query against the index (host/match.hpp, kernels/match.hpp) ----

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
    return sa::match_host(*ix, Q, m, max_len, false, ML, POS, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_match_stats_device(const sa_amd_index *ix, const uint8_t *dQ, int32_t m, int32_t max_len, uint32_t *dML,
                                                  uint32_t *dPOS, void *dWork, int64_t work_bytes, void *stream)
{
    if (!ix || m < 0 || max_len < 1 || (m > 0 && !dQ)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_device(*ix, dQ, m, max_len, false, dML, dPOS, nullptr, 0, nullptr, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_match_spans(const sa_amd_index *ix, const uint8_t *Q, int32_t m, int32_t min_len, uint32_t *spans,
                                           int64_t capacity, int64_t *count_out)
{
    if (!ix || m < 0 || min_len < 1 || (m > 0 && !Q) || capacity < 0 || !count_out || (capacity > 0 && !spans)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_host(*ix, Q, m, min_len, true, nullptr, nullptr, spans, capacity, count_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_match_spans_device(const sa_amd_index *ix, const uint8_t *dQ, int32_t m, int32_t min_len, uint32_t *dSpans,
                                                  int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes, void *stream)
{
    if (!ix || m < 0 || min_len < 1 || (m > 0 && !dQ) || capacity < 0 || !count_out || (capacity > 0 && !dSpans)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    return sa::match_device(*ix, dQ, m, min_len, true, nullptr, nullptr, dSpans, capacity, count_out, dWork, work_bytes,
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

SA_EXPORT int64_t sa_amd_docs_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::docs_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_index_set_documents(sa_amd_index *ix, const uint32_t *doc_off, int64_t ndocs)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::docs_valid(doc_off, ndocs) || doc_off[ndocs] != (uint32_t)ix->n) return SA_AMD_EINVAL;
    return sa::docs_set(*ix, doc_off, ndocs);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_of(const sa_amd_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || count < 0 || (count > 0 && (!pos || !doc_out)) || !ix->doc_off()) return SA_AMD_EINVAL;
    if (count == 0) return SA_AMD_OK;
    return sa::doc_of_host(*ix, pos, count, doc_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_of_device(const sa_amd_index *ix, const uint32_t *dPos, int64_t count, uint32_t *dDoc, void *stream)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || count < 0 || (count > 0 && (!dPos || !dDoc)) || ((((uintptr_t)dPos) | ((uintptr_t)dDoc)) & 3u) || !ix->doc_off()) return SA_AMD_EINVAL;
    if (count == 0) return SA_AMD_OK;
    return sa::doc_of_device(*ix, dPos, count, dDoc, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_search(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, uint32_t *occ,
                                          uint32_t *df)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count) || !ix->doc_off()) return SA_AMD_EINVAL;
    return sa::docs_query(*ix, pat_data, pat_off, count, false, occ, df, nullptr, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_list(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int64_t *list_off,
                                        uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count)) return SA_AMD_EINVAL;
    if (capacity < 0 || !list_off || !total_out || (capacity > 0 && !docs) || !ix->doc_off()) return SA_AMD_EINVAL;
    return sa::docs_query(*ix, pat_data, pat_off, count, true, nullptr, nullptr, list_off, docs, capacity, total_out);
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

// ---- Boolean document queries (host/doc_match.hpp, kernels/doc_match.hpp) ----

SA_EXPORT int32_t sa_amd_index_doc_match(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t npat, const int32_t *clause_off,
                                         const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off, int32_t nqueries, uint32_t *df,
                                         uint32_t *clause_df)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::doc_match_args_valid(pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries)) return SA_AMD_EINVAL;
    if (!ix->doc_off()) return SA_AMD_EINVAL;
    return sa::doc_match_query(*ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, false, df, clause_df, nullptr,
                               nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_match_list(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t npat,
                                              const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off,
                                              int32_t nqueries, int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::doc_match_args_valid(pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries)) return SA_AMD_EINVAL;
    if (capacity < 0 || !list_off || !total_out || (capacity > 0 && !docs) || !ix->doc_off()) return SA_AMD_EINVAL;
    return sa::doc_match_query(*ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, true, nullptr, nullptr, list_off,
                               docs, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_doc_match_stats(sa_amd_doc_match_stats *out)
{
    if (out) *out = sa::g_last_doc_match_stats;
}

SA_EXPORT int64_t sa_amd_doc_match_set_budget(int64_t bytes)
{
    const int64_t prev = sa::g_dm_budget < 0 ? sa::DM_BUDGET_DEFAULT : sa::g_dm_budget;
    sa::g_dm_budget = bytes < 0 ? -1 : (bytes < sa::DM_BUDGET_MIN ? sa::DM_BUDGET_MIN : (bytes > sa::DM_BUDGET_MAX ? sa::DM_BUDGET_MAX : bytes));
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
    if (!ix || !ix->doc_off() || !sa::docrep_args_valid(min_len, mode, scope, spans, capacity, count_out)) return SA_AMD_EINVAL;
    return sa::doc_repeats_index(*ix, min_len, mode, scope, spans, capacity, count_out, doc_bytes);
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
    if (!ix || !ix->doc_off()) return SA_AMD_EINVAL;
    return sa::docs_freq_enable(*ix);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_tf(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int64_t *list_off,
                                      uint32_t *docs, uint32_t *tf, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    // (in this order: everything that can be refused without the index is, before the index is looked at)
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count) || capacity < 0 || !list_off || !total_out) return SA_AMD_EINVAL;
    if (!ix->doc_off() || !ix->doc_slots()) return SA_AMD_EINVAL;
    return sa::doc_tf_query(*ix, pat_data, pat_off, count, 0, list_off, docs, tf, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_doc_topk(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int32_t k,
                                        int64_t *top_off, uint32_t *docs, uint32_t *tf)
{
    SA_ABI_GUARD_BEGIN
    // (in this order: everything that can be refused without the index is, before the index is looked at)
    if (!ix || k < 1 || k > SA_AMD_DOC_TOPK_MAX || !sa::search_patterns_valid(pat_data, pat_off, count) || !top_off) return SA_AMD_EINVAL;
    if (!ix->doc_off() || !ix->doc_slots()) return SA_AMD_EINVAL;
    return sa::doc_tf_query(*ix, pat_data, pat_off, count, k, top_off, docs, tf, 0, nullptr);
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

// ---- repeated substrings (host/substrings.hpp, kernels/substrings.hpp) ----

SA_EXPORT int64_t sa_amd_substrings_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::sub_layout(n).bytes;
}

SA_EXPORT int64_t sa_amd_substrings_bound(int32_t n)
{
    if (n < 0) return -1;
    return sa::substrings_bound(n);
}

SA_EXPORT int32_t sa_amd_substrings_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, const sa_amd_substr_query *query, uint32_t *dRows,
                                           uint32_t *dPos, int64_t capacity, int64_t *total, void *dWork, int64_t work_bytes, void *stream)
{
    if (n < 0 || !dSA || !dWork || (n > 0 && !dT)) return SA_AMD_EINVAL;
    SA_ABI_GUARD_BEGIN
    return sa::substrings_device(dT, dSA, n, query, dRows, dPos, capacity, total, dWork, work_bytes, (hipStream_t)stream);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_substrings(const uint8_t *T, int32_t n, const uint32_t *SA, const sa_amd_substr_query *query, uint32_t *rows,
                                    uint32_t *pos, int64_t capacity, int64_t *total)
{
    SA_ABI_GUARD_BEGIN
    return sa::substrings_host(T, n, SA, query, rows, pos, capacity, total);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_substrings(const sa_amd_index *ix, const sa_amd_substr_query *query, uint32_t *rows, uint32_t *pos,
                                          int64_t capacity, int64_t *total)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::substrings_index(*ix, query, rows, pos, capacity, total);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_substr_stats(sa_amd_substr_stats *out)
{
    if (out) *out = sa::g_last_substr_stats;
}

// ---- repeated substrings with their document frequency (host/doc_substrings.hpp, kernels/doc_substrings.hpp) ----

SA_EXPORT int64_t sa_amd_doc_substrings_work_bytes(int32_t n)
{
    if (n < 0) return -1;
    return (int64_t)sa::dsub_layout(n).bytes;
}

SA_EXPORT int32_t sa_amd_index_doc_substrings(const sa_amd_index *ix, const sa_amd_doc_substr_query *query, uint32_t *rows, uint32_t *df,
                                              uint32_t *pos, int64_t capacity, int64_t *total)
{
    SA_ABI_GUARD_BEGIN
    if (!ix) return SA_AMD_EINVAL;
    return sa::doc_substrings_index(*ix, query, rows, df, pos, capacity, total);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_doc_substr_stats(sa_amd_doc_substr_stats *out)
{
    if (out) *out = sa::g_last_doc_substr_stats;
}

// ---- n-gram / infinity-gram queries (host/ngram.hpp, kernels/ngram.hpp) ----

SA_EXPORT int32_t sa_amd_index_next_bytes(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, uint32_t *range_lo,
                                          uint32_t *range_hi, uint8_t *at_end, int64_t *list_off, uint8_t *bytes, uint32_t *counts, int64_t capacity,
                                          int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count) || capacity < 0) return SA_AMD_EINVAL;
    return sa::ngram_query(*ix, pat_data, pat_off, count, false, 1, 0, nullptr, range_lo, range_hi, at_end, list_off, bytes, counts, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_infgram(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int32_t min_count,
                                       int32_t max_len, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end, int64_t *list_off,
                                       uint8_t *bytes, uint32_t *counts, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::search_patterns_valid(pat_data, pat_off, count) || capacity < 0 || min_count < 1) return SA_AMD_EINVAL;
    return sa::ngram_query(*ix, pat_data, pat_off, count, true, min_count, max_len, suffix_len, range_lo, range_hi, at_end, list_off, bytes, counts,
                           capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_ngram_stats(sa_amd_ngram_stats *out)
{
    if (out) *out = sa::g_last_ngram_stats;
}

SA_EXPORT int32_t sa_amd_ngram_set_stream_cap(int32_t slots)
{
    const int32_t prev = sa::g_ngram_stream_cap < 0 ? sa::NG_STREAM_CAP_DEFAULT : sa::g_ngram_stream_cap;
    sa::g_ngram_stream_cap = slots < 0 ? -1 : (slots > sa::NG_STREAM_CAP_MAX ? sa::NG_STREAM_CAP_MAX : slots);
    return prev;
}

// ---- scoring a text under the infinity-gram model (host/score.hpp, kernels/score.hpp) ----

SA_EXPORT int64_t sa_amd_score_work_bytes(int64_t m, int64_t ndocs)
{
    if (m < 0 || ndocs < 0 || m > (int64_t)SA_AMD_MAX_LENGTH || ndocs > (int64_t)SA_AMD_MAX_LENGTH) return -1;
    return (int64_t)sa::score_layout(m, ndocs).bytes;
}

SA_EXPORT int32_t sa_amd_index_infgram_score(const sa_amd_index *ix, const uint8_t *Q, int64_t m, const int64_t *q_off, int64_t ndocs, int32_t min_count,
                                             int32_t max_len, uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END, uint32_t *NLO, uint32_t *NHI)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::score_args_valid(m, q_off, ndocs, min_count, max_len) || (m > 0 && !Q)) return SA_AMD_EINVAL;
    return sa::score_host(*ix, Q, m, q_off, ndocs, min_count, max_len, S, LO, HI, AT_END, NLO, NHI, sa::g_last_score_stats,
                          &sa_amd_score_stats::compared_bytes);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_index_infgram_score_device(const sa_amd_index *ix, const uint8_t *dQ, int64_t m, const int64_t *q_off, int64_t ndocs,
                                                    int32_t min_count, int32_t max_len, uint32_t *dS, uint32_t *dLO, uint32_t *dHI, uint8_t *dAT_END,
                                                    uint32_t *dNLO, uint32_t *dNHI, void *dWork, int64_t work_bytes, void *stream)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::score_args_valid(m, q_off, ndocs, min_count, max_len) || (m > 0 && !dQ)) return SA_AMD_EINVAL;
    sa::DeviceGuard guard(ix->device);
    if (guard.rc != SA_AMD_OK) return guard.rc;
    sa::ScoreOut out;
    out.S = dS; out.LO = dLO; out.HI = dHI; out.AT_END = dAT_END; out.NLO = dNLO; out.NHI = dNHI;
    return sa::score_device(*ix, dQ, m, q_off, ndocs, min_count, max_len, out, dWork, work_bytes, (hipStream_t)stream, sa::g_last_score_stats,
                            &sa_amd_score_stats::compared_bytes);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_score_stats(sa_amd_score_stats *out)
{
    if (out) *out = sa::g_last_score_stats;
}

SA_EXPORT int32_t sa_amd_score_set_group_cap(int32_t bytes)
{
    const int32_t prev = sa::g_score_cap < 0 ? sa::SCORE_CAP_DEFAULT : sa::g_score_cap;
    sa::g_score_cap = bytes < 0 ? -1 : (bytes > sa::SCORE_CAP_MAX ? sa::SCORE_CAP_MAX : bytes);
    return prev;
}

// ---- 16-bit token texts: construction, the token index and its queries (host/tokens.hpp, kernels/tokens.hpp) ----

SA_EXPORT int32_t sa_amd_max_tokens_u16(void) { return sa::TOK_MAX_TOKENS_U16; }

SA_EXPORT int32_t sa_amd_saca_u16(const uint16_t *T, uint32_t *SA, int32_t n)
{
    if (n < 0 || n > sa::TOK_MAX_TOKENS_U16 || !SA || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (n == 0) { SA[0] = 0; return SA_AMD_OK; }
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    return sa::tok_saca_host(T, SA, n);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_create(const uint16_t *T, int32_t n, const uint32_t *SA, sa_amd_tok_index **out)
{
    if (!out || n < 0 || n > sa::TOK_MAX_TOKENS_U16 || (n > 0 && !T)) return SA_AMD_EINVAL;
    *out = nullptr;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    return sa::tok_index_create(T, n, SA, out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_tok_index_destroy(sa_amd_tok_index *ix)      // (frees and deletes: nothing that throws, no change of device)
{
    delete ix;
}

SA_EXPORT int32_t sa_amd_tok_index_sa(const sa_amd_tok_index *ix, uint32_t *SA_out)
{
    if (!ix || !SA_out) return SA_AMD_EINVAL;
    return sa::tok_index_sa(*ix, SA_out);
}

SA_EXPORT int32_t sa_amd_tok_index_search(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                          uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::tok_patterns_valid(pat_data, pat_off, count)) return SA_AMD_EINVAL;
    return sa::tok_search(*ix, pat_data, pat_off, count, contains, range_lo, range_hi);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_next_tokens(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                               uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end, int64_t *list_off, uint16_t *tokens,
                                               uint32_t *counts, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::tok_patterns_valid(pat_data, pat_off, count) || capacity < 0) return SA_AMD_EINVAL;
    return sa::tok_query(*ix, pat_data, pat_off, count, false, 1, 0, nullptr, range_lo, range_hi, at_end, list_off, tokens, counts, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_infgram(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                           int32_t min_count, int32_t max_len, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi,
                                           uint8_t *at_end, int64_t *list_off, uint16_t *tokens, uint32_t *counts, int64_t capacity,
                                           int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::tok_patterns_valid(pat_data, pat_off, count) || capacity < 0 || min_count < 1) return SA_AMD_EINVAL;
    return sa::tok_query(*ix, pat_data, pat_off, count, true, min_count, max_len, suffix_len, range_lo, range_hi, at_end, list_off, tokens, counts,
                         capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_tok_stats(sa_amd_tok_stats *out)
{
    if (out) *out = sa::g_last_tok_stats;
}

SA_EXPORT int32_t sa_amd_tok_index_infgram_score(const sa_amd_tok_index *ix, const uint16_t *Q, int64_t m, const int64_t *q_off, int64_t ndocs,
                                                 int32_t min_count, int32_t max_len, uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END,
                                                 uint32_t *NLO, uint32_t *NHI)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::score_args_valid(m, q_off, ndocs, min_count, max_len) || (m > 0 && (!Q || ((uintptr_t)Q & 1u)))) return SA_AMD_EINVAL;
    return sa::score_host(*ix, Q, m, q_off, ndocs, min_count, max_len, S, LO, HI, AT_END, NLO, NHI, sa::g_last_tok_score_stats,
                          &sa_amd_tok_score_stats::compared_tokens);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_last_tok_score_stats(sa_amd_tok_score_stats *out)
{
    if (out) *out = sa::g_last_tok_score_stats;
}

// ---- 32-bit token texts, ids below 2^24: the same routes at Sym = uint32_t.  The statistics are the
//      calling thread's sa_amd_last_tok_stats / sa_amd_last_tok_score_stats, whichever width its latest token call had ----

SA_EXPORT int32_t sa_amd_max_tokens_u32(void) { return sa::TOK_MAX_TOKENS_U32; }

SA_EXPORT int32_t sa_amd_saca_u32(const uint32_t *T, uint32_t *SA, int32_t n)
{
    if (n < 0 || n > sa::TOK_MAX_TOKENS_U32 || !SA || (n > 0 && !T)) return SA_AMD_EINVAL;
    if (n == 0) { SA[0] = 0; return SA_AMD_OK; }
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    return sa::tok_saca_host(T, SA, n);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_create(const uint32_t *T, int32_t n, const uint32_t *SA, sa_amd_tok32_index **out)
{
    if (!out || n < 0 || n > sa::TOK_MAX_TOKENS_U32 || (n > 0 && !T)) return SA_AMD_EINVAL;
    *out = nullptr;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    SA_ABI_GUARD_BEGIN
    return sa::tok_index_create(T, n, SA, out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT void sa_amd_tok32_index_destroy(sa_amd_tok32_index *ix)  // (frees and deletes: nothing that throws, no change of device)
{
    delete ix;
}

SA_EXPORT int32_t sa_amd_tok32_index_sa(const sa_amd_tok32_index *ix, uint32_t *SA_out)
{
    if (!ix || !SA_out) return SA_AMD_EINVAL;
    return sa::tok_index_sa(*ix, SA_out);
}

SA_EXPORT int32_t sa_amd_tok32_index_search(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                            uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi)
{
    SA_ABI_GUARD_BEGIN
    if (const int32_t rc = sa::tok_query_args(ix, pat_data, pat_off, count)) return rc;
    return sa::tok_search(*ix, pat_data, pat_off, count, contains, range_lo, range_hi);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_next_tokens(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                                 uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end, int64_t *list_off, uint32_t *tokens,
                                                 uint32_t *counts, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (capacity < 0) return SA_AMD_EINVAL;
    if (const int32_t rc = sa::tok_query_args(ix, pat_data, pat_off, count)) return rc;
    return sa::tok_query(*ix, pat_data, pat_off, count, false, 1, 0, nullptr, range_lo, range_hi, at_end, list_off, tokens, counts, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_infgram(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                             int32_t min_count, int32_t max_len, uint32_t *suffix_len, uint32_t *range_lo, uint32_t *range_hi,
                                             uint8_t *at_end, int64_t *list_off, uint32_t *tokens, uint32_t *counts, int64_t capacity,
                                             int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    if (capacity < 0 || min_count < 1) return SA_AMD_EINVAL;
    if (const int32_t rc = sa::tok_query_args(ix, pat_data, pat_off, count)) return rc;
    return sa::tok_query(*ix, pat_data, pat_off, count, true, min_count, max_len, suffix_len, range_lo, range_hi, at_end, list_off, tokens, counts,
                         capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_infgram_score(const sa_amd_tok32_index *ix, const uint32_t *Q, int64_t m, const int64_t *q_off, int64_t ndocs,
                                                   int32_t min_count, int32_t max_len, uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END,
                                                   uint32_t *NLO, uint32_t *NHI)
{
    SA_ABI_GUARD_BEGIN
    if (!ix || !sa::score_args_valid(m, q_off, ndocs, min_count, max_len) || (m > 0 && (!Q || ((uintptr_t)Q & 3u)))) return SA_AMD_EINVAL;
    if (!sa::tok_ids_valid(Q, m)) return SA_AMD_ERANGE;
    return sa::score_host(*ix, Q, m, q_off, ndocs, min_count, max_len, S, LO, HI, AT_END, NLO, NHI, sa::g_last_tok_score_stats,
                          &sa_amd_tok_score_stats::compared_tokens);
    SA_ABI_GUARD_END(0)
}

// ---- document collections over the token indexes (include/sa_amd_tokdocs.h): the checks are
//      host/tokens.hpp's, the routes host/docs.hpp's and host/doc_match.hpp's on the token index types ----

SA_EXPORT int32_t sa_amd_tok_index_set_documents(sa_amd_tok_index *ix, const uint32_t *doc_off, int64_t ndocs)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_set(ix, doc_off, ndocs);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_set_documents_by_separator(sa_amd_tok_index *ix, uint32_t separator, int64_t *ndocs_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_set_by_separator(ix, separator, ndocs_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_doc_offsets(const sa_amd_tok_index *ix, uint32_t *doc_off_out, int64_t capacity, int64_t *ndocs_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_offsets(ix, doc_off_out, capacity, ndocs_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_doc_of(const sa_amd_tok_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_doc_of(ix, pos, count, doc_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_doc_search(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count, uint32_t *occ,
                                              uint32_t *df)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_query(ix, pat_data, pat_off, count, false, occ, df, nullptr, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_doc_list(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                            int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_query(ix, pat_data, pat_off, count, true, nullptr, nullptr, list_off, docs, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_doc_match(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t npat,
                                             const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off,
                                             int32_t nqueries, uint32_t *df, uint32_t *clause_df)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_match(ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, false, df, clause_df, nullptr,
                             nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok_index_doc_match_list(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t npat,
                                                  const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off,
                                                  int32_t nqueries, int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_match(ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, true, nullptr, nullptr, list_off,
                             docs, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_set_documents(sa_amd_tok32_index *ix, const uint32_t *doc_off, int64_t ndocs)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_set(ix, doc_off, ndocs);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_set_documents_by_separator(sa_amd_tok32_index *ix, uint32_t separator, int64_t *ndocs_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_set_by_separator(ix, separator, ndocs_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_doc_offsets(const sa_amd_tok32_index *ix, uint32_t *doc_off_out, int64_t capacity, int64_t *ndocs_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_offsets(ix, doc_off_out, capacity, ndocs_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_doc_of(const sa_amd_tok32_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_doc_of(ix, pos, count, doc_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_doc_search(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                                uint32_t *occ, uint32_t *df)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_query(ix, pat_data, pat_off, count, false, occ, df, nullptr, nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_doc_list(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                              int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_query(ix, pat_data, pat_off, count, true, nullptr, nullptr, list_off, docs, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_doc_match(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t npat,
                                               const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses, const int32_t *query_off,
                                               int32_t nqueries, uint32_t *df, uint32_t *clause_df)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_match(ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, false, df, clause_df, nullptr,
                             nullptr, 0, nullptr);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_tok32_index_doc_match_list(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t npat,
                                                    const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                                                    const int32_t *query_off, int32_t nqueries, int64_t *list_off, uint32_t *docs, int64_t capacity,
                                                    int64_t *total_out)
{
    SA_ABI_GUARD_BEGIN
    return sa::tokdocs_match(ix, pat_data, pat_off, npat, clause_off, clause_flags, nclauses, query_off, nqueries, true, nullptr, nullptr, list_off,
                             docs, capacity, total_out);
    SA_ABI_GUARD_END(0)
}

// ---- packed format (reference src/packed_sa.rs); byte layout: u32 magic "SA4x" LE, u32 length, u64 data length
//      (bincode's Vec<u8> prefix), data ----

SA_EXPORT int64_t sa_amd_pack_bound(int64_t length)
{
    if (length < 0 || length > 0xffffffffLL) return -1;
    return sa::pack_bound(length);
}

SA_EXPORT int32_t sa_amd_pack(const uint32_t *SA, int64_t length, uint8_t *out, int64_t capacity, int64_t *out_len)
{
    SA_ABI_GUARD_BEGIN
    return sa::pack(SA, length, out, capacity, out_len);
    SA_ABI_GUARD_END(0)
}

SA_EXPORT int32_t sa_amd_unpack(const uint8_t *bytes, int64_t nbytes, uint32_t *SA, int64_t capacity, int64_t *length)
{
    SA_ABI_GUARD_BEGIN
    return sa::unpack(bytes, nbytes, SA, capacity, length);
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

SA_EXPORT int32_t sa_amd_device_count(void) { return sa::device_count(); }

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
