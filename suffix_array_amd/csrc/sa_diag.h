/*
 * sa_diag.h -- entry points of libsuffix_array_amd_diag.so ONLY (built with -DSA_AMD_DIAG from the same sources as the
 * product library).  The diagnostic library additionally honours SA_AMD_SORT_VARIANT values that select timing
 * ablations (kernels that skip ranking or stores and therefore produce WRONG orders) and
 * SA_AMD_TIMING_ONLY_INITIAL_SORT (stops after the initial sort).  None of that exists in libsuffix_array_amd.so.
 * Users: tools/ (profiles/*ablation*, phase stamps) and the primitive tests of tests/test_gpu_parity.py.
 */
#ifndef SUFFIX_ARRAY_AMD_DIAG_H
#define SUFFIX_ARRAY_AMD_DIAG_H
#include "../../include/suffix_array_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
/* cycles per phase of the stamped kernels, summed over tiles and workgroups; reading zeroes the counters */
int32_t sa_amd_debug_phase_cycles(uint64_t *out, int32_t count);
/* k_group_sort: switch its per-phase stamps on / off (entries 8..13 of the same array) */
int32_t sa_amd_debug_group_sort_stamps(int32_t on);
/* k_rr_count: switch its per-phase stamps on / off (entries 0..7 of the same array; tools/rr_count_stamps.py) */
int32_t sa_amd_debug_rr_count_stamps(int32_t on);
/* the old forms of the dense route's re-rank writes, for A/B and the route tests (process-wide; returns the previous flags):
 * bit 0: dense rounds write SA for every listed suffix each round (not only in the round it leaves the list),
 * bit 1: the binned rank set-up copies SA into its pair keys (instead of binning straight from the suffix array) */
int32_t sa_amd_debug_rerank_routes(int32_t flags);
/* when the last pass of the 64-bit initial sort writes group-start flags instead of the sorted keys (process-wide; returns the
 * previous mode): 0 never (the key route), 1 when the dense route is expected (what the product library always does), 2 whenever
 * that sort runs -- the routes that read the sorted keys then rebuild them.  Every mode gives the same array and statistics. */
int32_t sa_amd_debug_head_flags(int32_t mode);
/* whether a dense doubling round hands its re-rank one status byte per list member instead of the 8-byte keys (process-wide;
 * returns the previous mode): 0 never (the key route), 1 where a dead device-resident slab exists for the bytes (what the product
 * library always does), 2 the same with the round's key buffer and status slab filled with a poison pattern before the local
 * pass, so that a read of an entry the round never wrote changes the result.  Every mode gives the same array and statistics. */
int32_t sa_amd_debug_round_flags(int32_t mode);
/* the second bound of the term-frequency kernel (process-wide; returns the previous mode): 0 galloping from the first bound (what
 * the product library always does), 1 a plain binary search of the document's part.  Both give the same answers. */
int32_t sa_amd_debug_doc_tf_bounds(int32_t mode);
/* the pair pass of sa_amd_index_doc_substrings (process-wide; returns the previous mode): 0 equal targets inside a wave are
 * combined into one atomic (what the product library always does), 1 one atomic per pair.  Both give the same table. */
int32_t sa_amd_debug_dsub_plain_atomics(int32_t mode);
/* what recycled memory holds when a route gets it (process-wide; returns the previous pattern): -1 off (the default: the bytes
 * are whatever the last user left, as in the product library), 0 .. 255 every byte takes that value, 256 "small": 32-bit word i
 * is mix(i + seed) % 5 -- in range as an index, a count or a flag of every table, so that a stale read is a wrong answer and no
 * wild address --, 257 "random": word i is mix(i + seed).  While it is on, the fill is applied, and waited for, before the first
 * use of: the bytes asked of the pool for every pooled device block (the derived-array and query routes, the build of the
 * host-pointer path on its full and its reduced-memory route, the pinned spill of the latter included); the pinned blocks the
 * small-text and small-batch kernels read and write zero-copy; every allocation an index or a token index owns, the slack
 * behind its text included.  The contract it tests: no result and no statistic depends on those bytes. */
int32_t sa_amd_debug_fill_blocks(int32_t pattern);
/* Refused allocations.  All memory the library takes goes through three seams: a pooled device block
 * (ResourcePool::acquire), a pinned host block (ResourcePool::pinned) and a table of an index or a buffer of a host form
 * (DevBuf::alloc).  Each seam counts a request at its top, on the thread that calls it: before the pool looks for a free block
 * and before a pinned block's allocation is handed to a helper thread, so the count depends neither on what the pool holds nor
 * on the thread that ends up calling the runtime.  The switch acts on the CALLING THREAD only: nth >= 1: the nth request this
 * thread makes from now on is refused, once; 0: count only; -1: off (the default: nothing is counted).  Returns the number of
 * requests this thread made since the previous call of this function.  A refused request asks the runtime for more bytes than
 * any device has (SIZE_MAX / 2) and returns what the seam returns for that answer, without touching the pool: the runtime
 * refuses on the host, nobody's memory is taken, and the thread is left as a real refusal leaves it.  Requests made by helper
 * and worker threads (the early pullers of a download, the workers of sa_amd_saca_batch) belong to those threads, not to the
 * thread that armed the switch: they are neither counted nor refused.  Stream and event creation are no memory requests (they
 * fail with SA_AMD_EHIP) and are out of this switch's reach. */
int32_t sa_amd_debug_refuse_alloc(int32_t nth);
/* 1 when the refusal armed by the calling thread's last sa_amd_debug_refuse_alloc(nth >= 1) has happened, else 0 */
int32_t sa_amd_debug_refuse_fired(void);
/* the kinds of the requests counted since the calling thread last set the switch, in order: 1 a pooled device block, 2 a pinned
 * block, 3 a table / buffer (DevBuf); at most `capacity` (and at most 64) are written; returns the number of requests counted */
int32_t sa_amd_debug_refuse_kinds(uint8_t *kinds, int32_t capacity);
/* the ledger (process-wide): allocations made through the three seams and not yet given back to the runtime at one of the seven
 * hipFree / hipHostFree sites (pool.hpp, support.hpp) -- blocks the pool retains are live; sa_amd_release_cache frees them */
int32_t sa_amd_debug_live_allocations(int64_t *device, int64_t *pinned);
int32_t sa_amd_debug_sort_variant_count(void);
const char *sa_amd_debug_sort_variant_name(int32_t index);
/* stable LSD radix sort of (u64 key, u32 value) pairs on bits [begin_bit, end_bit); host buffers */
int32_t sa_amd_test_sort_pairs(uint64_t *keys, uint32_t *vals, int64_t count, int32_t begin_bit, int32_t end_bit);
/* the same sort (single-pass engine) with the flags variant of its last pass: vals = the sorted order; flags_out[count] = one byte
 * per output position p: 0 = p continues the group (run of equal keys) of p - 1, 1 = p starts a group, 2 = compare
 * keys_out[p] with keys_out[p - 1] (both are true sorted keys there); keys_out[count] = that pass's key buffer, 0xA5 bytes wherever
 * the pass stored nothing; keys is read only */
int32_t sa_amd_test_sort_pairs_flags(const uint64_t *keys, uint32_t *vals, int64_t count, int32_t begin_bit, int32_t end_bit,
                                     uint8_t *flags_out, uint64_t *keys_out);
/* the sample sort of the 64-bit stage (kernels/sample_sort.hpp; count >= 262 144): keys in order out, vals[i] = the index key i came
 * from; *done = 0: a bucket that is no equality bucket did not fit a workgroup -- the pipeline then takes the LSD sort */
int32_t sa_amd_test_sample_sort64(uint64_t *keys, uint32_t *vals, int64_t count, int32_t key_bits, int32_t *done);
/* the 32-bit-key form of the same sort (first stage of the two-stage initial sort) */
int32_t sa_amd_test_sort_pairs32(uint32_t *keys, uint32_t *vals, int64_t count, int32_t begin_bit, int32_t end_bit);
/* stage 1 of the Lempel-Ziv factorisation alone: nearest smaller values of a DEVICE array of distinct values (see sa_diag.inc) */
int32_t sa_amd_test_lz_nsv(const uint32_t *dA, int64_t n, uint32_t *dPsv, uint32_t *dNsv, int64_t *counters);
/* the same order through two global passes over the top 16 (or 18: nine-bit digits) key bits + the in-LDS bucket sort of the
 * rest (kernels/bucket_sort.hpp); *largest = the largest bucket; returns 1 (buffers untouched) when no workgroup shape holds it */
int32_t sa_amd_test_bucket_sort32(uint32_t *keys, uint32_t *vals, int64_t count, int32_t top_bits, uint32_t *largest);
/* initial packed keys of a text (host buffers; keys has n entries); returns bits in *bits, symbols in *k */
int32_t sa_amd_test_build_keys(const uint8_t *T, int32_t n, uint64_t *keys, int32_t *bits, int32_t *k);
/* micro-prototype for DESIGN.md section 2 / VERDICT r1 row (g): one exact level-0 L-type induce sweep of SA-IS executed by a
 * single wavefront with the bucket heads in LDS; SA (n + 1 slots) holds the LMS suffixes at their places and 0xffffffff
 * elsewhere and is completed in place; typeL: bit j = suffix j is L-type; head: 256 bucket starts; counters[0] = induced
 * suffixes, counters[1] = 64-slot blocks that had to be re-read */
int32_t sa_amd_proto_induce_l(const uint8_t *T, const uint8_t *typeL, uint32_t *SA, int32_t n, const uint32_t *head,
                              double *ms, uint64_t *counters);
#ifdef __cplusplus
}
#endif
#endif
