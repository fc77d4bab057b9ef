/*
 * suffix_array_amd.h -- C ABI of the MI355X-native suffix-array construction engine.
 *
 * Drop-in boundary for ONE path of hucsmn/suffix_array: `SuffixArray::new(&[u8])`
 * -> `saca()` -> `cdivsufsort::sort_in_place`.  Citations are file:line in the reference
 * crate (v0.5.0).  Plain pointers and sizes only; no C++ or torch types cross this ABI.
 *
 * Output contract (reference src/saca.rs:9-15, src/sa.rs:72-84): the n non-empty suffixes of
 * T in ascending unsigned-lexicographic order (a proper prefix sorts first), as start offsets.
 * All suffixes are distinct, so the array is unique: the result is bit-identical to the
 * crate's divsufsort path on the same bytes.
 *
 * Every entry point is synchronous, thread-safe and re-entrant; the library keeps no pointer
 * to caller memory after returning and never writes past the stated output length.  There is
 * NO CPU fallback: without a usable HIP device the calls return SA_AMD_ENODEVICE.
 */
#ifndef SUFFIX_ARRAY_AMD_H
#define SUFFIX_ARRAY_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes; 0 / -1 / -2 keep the meaning of libdivsufsort's return value that the
 * reference's dependency asserts on (call site reference src/saca.rs:14) */
#define SA_AMD_OK          0
#define SA_AMD_EINVAL     (-1)   /* null pointer with n > 0, n < 0, bad device ordinal */
#define SA_AMD_ENOMEM     (-2)   /* host or device allocation failed */
#define SA_AMD_EHIP       (-3)   /* HIP runtime error (launch, copy, sync) */
#define SA_AMD_ENODEVICE  (-4)   /* no HIP device visible */
#define SA_AMD_EINTERNAL  (-5)   /* refinement did not converge (cannot happen for valid input) */
#define SA_AMD_ERANGE     (-6)   /* check_integrity: an entry exceeds n (the reference panics, src/sa.rs:77-78) */

/* reference src/saca.rs:6  `pub const MAX_LENGTH: usize = std::i32::MAX as usize;` */
#define SA_AMD_MAX_LENGTH 2147483647

/* reference src/saca.rs:6 as a callable, for FFI users that cannot read macros */
int32_t sa_amd_max_length(void);

/*
 * Replaces the C engine the reference binds: `int divsufsort(const unsigned char *T, int *SA,
 * int n)` behind `cdivsufsort::sort_in_place(&[u8], &mut [i32])` (reference src/saca.rs:3,14).
 * T: n bytes (host), any byte values.  SA: n entries (host), contents on entry arbitrary
 * (reference src/sa.rs:31 re-uses an old buffer).  n == 0 is a successful no-op.
 */
int32_t sa_amd_divsufsort(const uint8_t *T, int32_t *SA, int32_t n);

/*
 * Replaces `pub fn saca(s: &[u8], sa: &mut [u32])` itself (reference src/saca.rs:9-15):
 * SA has n + 1 entries, SA[0] = n (src/saca.rs:13), SA[1..=n] as above.  The two asserts of
 * src/saca.rs:10-11 become the caller's job (lengths are implied by n).
 * A refused allocation is SA_AMD_ENOMEM (after the reduced-memory route has been tried) with SA untouched, with one exception: the
 * front of a large array travels while the last rounds run, so a failing call can leave SA (partly) written once the early download has begun.
 */
int32_t sa_amd_saca_u8(const uint8_t *T, uint32_t *SA, int32_t n);

/*
 * Batch of independent texts, text i built on HIP device `device[i]` (NULL: i mod device
 * count), one host thread per device, no inter-device traffic.
 * status[i] receives the per-text code; the return value is the first non-zero status or 0.
 * Each SA[i] has n[i] + 1 entries (layout of sa_amd_saca_u8).
 * The texts of up to SA_AMD_SMALL_MAX (8192) bytes of a device are built together: one launch per chunk
 * of up to 96 MiB of them, one workgroup per text (a caller that indexes thousands of short strings, the
 * reference's own test domain src/tests.rs:13-17, pays ~0.04-1.6 us per text instead of 20-100 us per call).
 */
int32_t sa_amd_saca_batch(const uint8_t *const *T, uint32_t *const *SA, const int32_t *n,
                          const int32_t *device, int32_t count, int32_t *status);

/* ---- device-resident entry points (text already in HBM; used by bench.py) ----
 *
 * The `stream` of every `_device` form, here and below: any hipStream_t of the current device (of the index's device for the
 * sa_amd_index_* forms) -- NULL = the default stream, a blocking stream or a non-blocking one (hipStreamNonBlocking).
 *   Everything the call does on the device (kernels, clears of its control words, read-backs, sort passes, the copy of host
 *     arguments such as q_off) is queued on `stream` and on no other stream.
 *   So the call orders itself behind the work already queued on `stream`: inputs and a work block that are still being produced
 *     there need no synchronisation before the call.  Work on OTHER streams is not waited for; that is the caller's job.
 *   "Blocks until done": the call has waited for `stream` when it returns.  The outputs in device memory are complete and can be
 *     read from any stream without a further wait on `stream`; the host words (*count_out, *total, *primary_out, the return
 *     value, the statistics getters) are final.  Because the calls block they cannot be captured into a graph.
 */

typedef struct sa_amd_stats {
    int32_t sigma;            /* distinct byte values in T */
    int32_t bits_per_symbol;  /* packed code width when sigma is a power of two, 0 = base-sigma packing */
    int32_t symbols_per_key;  /* symbols in the initial 64-bit key */
    int32_t rounds;           /* prefix-doubling refinement rounds after the initial sort */
    int32_t sort_passes;      /* 8-bit radix passes executed in total */
    int32_t sparse_mode;      /* 1: few tied suffixes, ranks looked up in the sorted keys instead of a full ISA */
    int64_t sorted_elements;  /* sum over sort passes of elements moved */
    int64_t unresolved_after_initial; /* suffixes still in groups > 1 after the initial sort */
    int32_t text_rounds;      /* of `rounds`: text-keyed rounds (secondary key read from the text, no rank array) */
    int32_t top32_first;      /* 1: the entropy probe chose to sort on the top 32 key bits first and finish the ties locally */
    int64_t locally_sorted;   /* tied suffixes refined by the in-LDS group sort instead of the global radix sort */
    int32_t readbacks;        /* blocking device -> host read-backs of counters during the build (each one drains the stream) */
    int32_t reserved;
} sa_amd_stats;

/* bytes of device scratch sa_amd_saca_device needs for a text of n bytes */
int64_t sa_amd_workspace_bytes(int32_t n);

/*
 * dT: n bytes in device memory; dSA: n + 1 uint32 in device memory (layout of sa_amd_saca_u8);
 * dWork: sa_amd_workspace_bytes(n) bytes of device scratch, 256-byte aligned (else SA_AMD_EINVAL); stream: a
 * hipStream_t (NULL = default stream) on the current device.  Blocks until the array is
 * complete (the refinement loop reads a 4-byte counter back per round).  stats may be NULL.
 * dT may sit at any byte address; when it is not 4-byte aligned the kernels that read the text in words round the address
 * down and may READ (never write) up to three bytes in front of it -- inside the same device allocation, whose start is
 * aligned.
 */
int32_t sa_amd_saca_device(const uint8_t *dT, uint32_t *dSA, int32_t n, void *dWork,
                           int64_t work_bytes, void *stream, sa_amd_stats *stats);

/* The host-pointer entry points take their device memory (text + SA + workspace of one build = one block), streams and
 * pinned staging buffers from a process-wide pool, so repeated calls do not pay hipMalloc / hipFree; the pool retains at
 * most SA_AMD_CACHE_MAX_BYTES of device memory (default 128 GiB of the 288 GB).  This empties the pool now. */
void sa_amd_release_cache(void);

/* wall-clock phases of the calling thread's most recent host-pointer build, milliseconds:
 * [0] acquire device block + stream, [1] text upload, [2] build on the device, [3] suffix array download,
 * [4] release, [5] total, [6] helper threads of the staged download (0 = one plain hipMemcpy), [7] the fraction of the
 * array that was copied to the host before the build was done (early download: large arrays whose last refinement rounds
 * touch few slots start travelling while those rounds run; [3] is then the time behind the build only), [8] bytes of the
 * workspace that lived in pinned host memory (reduced-memory route: the device could not give the whole workspace).  Returns 9. */
int32_t sa_amd_last_host_timing(double *ms, int32_t capacity);

/* statistics of the most recent build issued by the calling thread (any entry point) */
void sa_amd_last_stats(sa_amd_stats *out);

/* number of visible HIP devices (0 when none; never initialises a context by itself) */
int32_t sa_amd_device_count(void);
/* PCI address ("0000:c1:00.0") of HIP device `device` into buf (capacity >= 16): which physical GPU an ordinal is -- bench.py
 * prints it per rank so that an N-GPU run can be seen to have used N distinct GPUs */
int32_t sa_amd_device_pci_bus_id(int32_t device, char *buf, int32_t capacity);

const char *sa_amd_strerror(int32_t code);
const char *sa_amd_version(void);

/* ---- next rows, on either side of the construction path ----
 *
 * Bucket table of `enable_buckets` (reference src/sa.rs:89-119): 256 * 257 + 1 = 65 793 entries in the
 * layout of src/sa.rs:94; bkt[i] = exclusive right edge of bucket i inside the SA (what the reference
 * gets by counting bigrams, src/sa.rs:100-108, and prefix-summing, src/sa.rs:112-116).  Built the same
 * way here -- from the TEXT alone: a bigram histogram kernel (two half tables of 32-bit LDS counters per
 * pair of workgroups) and one scan; only the text is uploaded (n bytes), 257 KiB come back.
 */
#define SA_AMD_BUCKET_TABLE_LEN 65793
/* T: n bytes, bkt: 65 793 entries; host buffers.  SA is not read (the reference's enable_buckets never touches the
 * array either) and may be NULL; the parameter stays for callers of the earlier form */
int32_t sa_amd_bucket_table(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *bkt);
/* SuffixArray::new followed by enable_buckets in one device round trip (the text is uploaded once).  A refused allocation is
 * SA_AMD_ENOMEM with neither SA nor bkt written: outputs are written only after the last step that can fail. */
int32_t sa_amd_saca_u8_buckets(const uint8_t *T, uint32_t *SA, int32_t n, uint32_t *bkt);
/* dSA == NULL: from the text alone (bigram counts; dBkt doubles as the scratch); dSA = a valid device-resident suffix
 * array of dT: one binary search per bucket edge instead (what sa_amd_index_buckets uses) */
int32_t sa_amd_bucket_table_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dBkt, void *stream);

/*
 * `check_integrity` (reference src/sa.rs:72-84), the validation behind `from_parts` and every
 * `load*` (src/sa.rs:57-64, :293-361), in linear time: returns 1 (true), 0 (false; also when
 * sa_len != n + 1, src/sa.rs:73-75), SA_AMD_ERANGE when an entry exceeds n (the reference panics
 * on the slice index there), or another negative status.  dWork: at least 4 * (n + 1) + 256 bytes
 * (random-store inverse permutation); with sa_amd_check_integrity_work_bytes(n) bytes, 256-byte
 * aligned, and a 16-byte aligned dSA the check runs at streaming cost (binned inverse permutation,
 * one random rank line per slot: 25 -> ~10 ms at 256 MiB).
 * Empty text (n == 0): SA = {0} gives 1 and any other single entry SA_AMD_ERANGE.  The reference returns
 * true there without reading the entry (its pair loop never runs); an index built on such an array
 * would read past the text, so the check rejects it like any other entry beyond n.
 */
int64_t sa_amd_check_integrity_work_bytes(int32_t n);
int32_t sa_amd_check_integrity(const uint8_t *T, int32_t n, const uint32_t *SA, int64_t sa_len);
int32_t sa_amd_check_integrity_device(const uint8_t *dT, int32_t n, const uint32_t *dSA, void *dWork,
                                      int64_t work_bytes, void *stream);

/*
 * Device-resident index: the text and its suffix array stay in HBM (SA == NULL: the array is built
 * there, i.e. SuffixArray::new without the 4(n+1)-byte download), then serve the bucket table, the
 * integrity check and BATCHED search -- `contains` / `search_all` / `search_lcp` of reference
 * src/sa.rs:164-253 (no-bucket paths) for `count` patterns per call, one wavefront per pattern.
 * Patterns are concatenated in pat_data; pattern q is pat_data[pat_off[q] .. pat_off[q+1]).
 * Outputs (any may be NULL), per pattern:
 *   contains[q]            1 iff the pattern occurs                            (src/sa.rs:164-170)
 *   range_lo/hi[q]         search_all(pat) == &sa[lo..hi]                      (src/sa.rs:173-204)
 *   lcp_start/len[q]       search_lcp(pat) == start..start+len                 (src/sa.rs:207-253)
 * A refused allocation is SA_AMD_ENOMEM, here and in every host-pointer and index entry point of this header: outputs are written
 * only after the last step that can fail (a table-building call leaves the index as it was), and the thread is left with no
 * pending runtime error.  The creating calls -- this one, sa_amd_tok_index_create, sa_amd_tok32_index_create -- are the exception
 * that protects the caller: a failing create sets *out to NULL, so that no caller is left with a dangling handle.  Where the refused request has a fallback -- the small integrity
 * block, the reduced-memory route of a build, the read-backs' pinned block -- the call succeeds with the same answers instead.
 * The other exceptions are named where they apply (sa_amd_unpack's *length; tf of sa_amd_index_doc_tf / _doc_topk; the array of a
 * build whose early download had begun, see sa_amd_saca_u8).
 */
typedef struct sa_amd_index sa_amd_index;
int32_t sa_amd_index_create(const uint8_t *T, int32_t n, const uint32_t *SA, sa_amd_index **out);
void sa_amd_index_destroy(sa_amd_index *ix);
int32_t sa_amd_index_sa(const sa_amd_index *ix, uint32_t *SA_out);               /* n + 1 entries */
int32_t sa_amd_index_buckets(sa_amd_index *ix, uint32_t *bkt);                   /* 65 793 entries; the index keeps the table and
                                                                                    later searches start from the pattern's bucket
                                                                                    (get_bucket, reference src/sa.rs:123-144) */
int32_t sa_amd_index_check_integrity(const sa_amd_index *ix);                    /* as sa_amd_check_integrity */
int32_t sa_amd_index_search(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count,
                            uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi, uint32_t *lcp_start,
                            uint32_t *lcp_len);

/*
 * Packed format of the `pack` feature (reference src/packed_sa.rs, src/sa.rs:255-361): header u32 magic
 * "SA4x" LE (src/packed_sa.rs:6-7), u32 length, u64 data length (bincode little-endian Vec<u8>), then the
 * suffix array bit-packed at ceil(log2(length)) bits in blocks of 128 (BitPacker4x), the last partial
 * block right-trimmed of zero bytes (src/packed_sa.rs:36-46).  PARITY UNPINNED at byte level: the block
 * layout is the external `bitpacking 0.8` crate's, restated from its published description; the
 * reference's own test pins the round trip only (src/tests.rs:61-76).
 * sa_amd_pack: SA has `length` entries, out has sa_amd_pack_bound(length) bytes; *out_len = bytes written.
 * sa_amd_unpack: *length receives the stored length; SA (capacity entries) receives the array.
 * A refused allocation is SA_AMD_ENOMEM; outputs are written only after the last step that can fail, with one exception, so that
 * a caller can size SA from a call that fails: *length receives the stored length as soon as the header has been read, also where the call then fails.
 */
int64_t sa_amd_pack_bound(int64_t length);
int32_t sa_amd_pack(const uint32_t *SA, int64_t length, uint8_t *out, int64_t capacity, int64_t *out_len);
int32_t sa_amd_unpack(const uint8_t *bytes, int64_t nbytes, uint32_t *SA, int64_t capacity, int64_t *length);

/*
 * LCP array (an extension: the reference lists it as a TODO, "construct enhanced suffix array"), aligned with the layout
 * of sa_amd_saca_u8: n + 1 entries, LCP[0] = 0, LCP[i] = length of the longest common prefix of the suffixes at SA[i-1]
 * and SA[i] (1 <= i <= n; LCP[1] = 0, the empty suffix), each at most n - 1.  Built on the device from the text and the
 * array by the permuted LCP (irreducible values compared directly, the rest by one max-scan): the bytes compared are at
 * most about 2 n log2 n whatever the LCP values.
 * SA must be the suffix array of T -- not proved here (sa_amd_check_integrity does that); an entry > n returns
 * SA_AMD_ERANGE (range pass before anything reads through the entries), SA[0] != n returns SA_AMD_EINVAL.
 */
/* bytes of device scratch sa_amd_lcp_device needs: at most sa_amd_check_integrity_work_bytes(n), about 20 (n + 1) */
int64_t sa_amd_lcp_work_bytes(int32_t n);
/* device pointers: dT n bytes (any byte address, read as sa_amd_saca_device reads it), dSA and dLCP n + 1 entries, dWork
 * sa_amd_lcp_work_bytes(n) bytes 256-byte aligned (else SA_AMD_EINVAL); stream a hipStream_t (NULL = default stream).
 * Blocks until done. */
int32_t sa_amd_lcp_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dLCP,
                          void *dWork, int64_t work_bytes, void *stream);
/* host pointers: T (n bytes) and SA (n + 1 entries) go up, LCP (n + 1 entries) comes back */
int32_t sa_amd_lcp(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *LCP);
/* sa_amd_saca_u8 and the LCP array in one device round trip: the array is built on the device and never uploaded */
int32_t sa_amd_saca_u8_lcp(const uint8_t *T, uint32_t *SA, int32_t n, uint32_t *LCP);
/* from the index's resident text and suffix array (n + 1 entries) */
int32_t sa_amd_index_lcp(const sa_amd_index *ix, uint32_t *LCP);

/*
 * Enhanced suffix array (an extension: the reference's README TODO "speed up searching by LCP array"), opt-in per index.
 * sa_amd_index_enable_lcp builds the LCP array of the resident text and array (as sa_amd_index_lcp, on the device), turns it
 * into the LCP table of a fixed search tree -- one uint64 per slot, 8 (n + 1) bytes kept in the index -- and drops the LCP
 * array.  A no-op when the index has the table; errors as sa_amd_index_lcp (SA_AMD_ERANGE, SA_AMD_EINVAL), SA_AMD_ENOMEM when
 * the table does not fit.  Later sa_amd_index_search calls take the LCP route: Manber-Myers search, at most
 * 2 plen + 128 log2 P text bytes compared per pattern (P the smallest power of two >= n + 2) instead of O(plen log n), with
 * answers identical to the plain route's, bucket table or not.  When the resident array is not the
 * suffix array of the text the answers are unspecified, but nothing is read outside the text, the patterns or the tables.
 */
int32_t sa_amd_index_enable_lcp(sa_amd_index *ix);

typedef struct sa_amd_search_stats {   /* of the calling thread's most recent sa_amd_index_search */
    int64_t patterns;                  /* patterns of that call */
    int64_t compared_bytes;            /* text bytes compared, every 64-byte chunk a wave loaded counted whole (LCP route) */
    int64_t steps;                     /* tree steps, 2 log2 P per pattern (LCP route) */
    int64_t table_steps;               /* steps decided from the table, without loading SA or the text (LCP route) */
    int32_t route;                     /* 0: plain binary search (the three counters above read -1), 1: LCP route */
    int32_t reserved;
} sa_amd_search_stats;
void sa_amd_last_search_stats(sa_amd_search_stats *out);

typedef struct sa_amd_lcp_stats {   /* of the calling thread's most recent LCP build */
    int64_t irreducible;            /* positions whose value was computed directly */
    int64_t compared_bytes;         /* text bytes loaded for comparison (both suffixes), short and long paths together */
    int64_t long_pairs;             /* pairs that went to the long-compare path (equal over the compare cap) */
    int32_t readbacks, reserved;    /* blocking device -> host read-backs of counters */
} sa_amd_lcp_stats;
void sa_amd_last_lcp_stats(sa_amd_lcp_stats *out);
/* route switch of the calling thread's later LCP builds (never changes a result): bytes one lane compares before a pair goes to
 * the long-compare path, clamped to 0 .. 1 048 576 (0: every irreducible pair takes it); a negative value restores the default
 * (64).  Returns the previous value. */
int32_t sa_amd_lcp_set_compare_cap(int32_t bytes);

/*
 * Burrows-Wheeler transform and its inverse (an extension of this crate's path; the group `divbwt` / `inverse_bw_transform`
 * of the C engine the reference binds).  libdivsufsort's sources are not part of this project, so the layout below is this
 * library's own contract, restated from the published description of divbwt and pinned by the tests.
 * With SA in the layout of sa_amd_saca_u8 (n + 1 entries, SA[0] = n):
 *   primary = the slot i with SA[i] == 0: 1 <= primary <= n for n > 0, and 0 for the empty text;
 *   B has n bytes: B[k] = T[SA[k] - 1] for k < primary and B[k] = T[SA[k + 1] - 1] for k >= primary.  So B[0] = T[n - 1], and
 *   the row of the whole text (where a sentinel would stand) is left out.  "banana" -> "annbaa", primary 4.
 * The inverse takes (B, n, primary) and returns T, for every byte string (zeros included).
 * Argument errors of the forward calls, as for the LCP array: a range pass runs before anything is read through the entries;
 * an entry > n is SA_AMD_ERANGE; SA[0] != n, or not exactly one entry equal to 0, is SA_AMD_EINVAL.  The array is not otherwise
 * proved to be the suffix array (sa_amd_check_integrity does that): with a wrong permutation the bytes of B are unspecified,
 * but nothing is read outside the text or written outside B.
 */
/* bytes of device scratch sa_amd_bwt_device needs (256, whatever n) */
int64_t sa_amd_bwt_work_bytes(int32_t n);
/* device pointers: dT n bytes (any byte address, read byte by byte), dSA n + 1 entries, dBWT n bytes (any byte address; may not
 * alias dT), dWork sa_amd_bwt_work_bytes(n) bytes 256-byte aligned (else SA_AMD_EINVAL), primary_out a HOST pointer; stream a
 * hipStream_t (NULL = default stream).  Blocks until done. */
int32_t sa_amd_bwt_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint8_t *dBWT, int32_t *primary_out,
                          void *dWork, int64_t work_bytes, void *stream);
/* host pointers.  SA == NULL: the array is built on the device, used there and never downloaded (divbwt(T, U, NULL, n)): n bytes
 * go up and n come back.  SA != NULL (n + 1 entries): the caller's array goes up instead of being rebuilt. */
int32_t sa_amd_bwt(const uint8_t *T, int32_t n, const uint32_t *SA, uint8_t *BWT, int32_t *primary_out);
/* from the index's resident text and suffix array */
int32_t sa_amd_index_bwt(const sa_amd_index *ix, uint8_t *BWT, int32_t *primary_out);

/*
 * Inverse: one stable 8-bit sort of the indices of B gives the row permutation psi; rows whose hash is 0 mod S (and `primary`)
 * are splitters; one lane per splitter walks psi to the next splitter, the sublists are ranked from primary's by pointer
 * jumping, and a second walk writes the text.  primary outside 1 .. n (0 for n = 0) is SA_AMD_EINVAL; a
 * pair (B, primary) that is not the transform of any text (the walk from primary closes before it has visited n + 1 rows) is
 * SA_AMD_EINVAL too: the call still terminates and has then written nothing to T_out.
 */
/* bytes of device scratch sa_amd_unbwt_device needs: about 16.5 (n + 1) */
int64_t sa_amd_unbwt_work_bytes(int32_t n);
/* device pointers: dBWT and dT_out n bytes each (any byte address), dWork sa_amd_unbwt_work_bytes(n) bytes 256-byte aligned (else
 * SA_AMD_EINVAL); stream a hipStream_t (NULL = default stream).  Blocks until done. */
int32_t sa_amd_unbwt_device(const uint8_t *dBWT, int32_t n, int32_t primary, uint8_t *dT_out, void *dWork,
                            int64_t work_bytes, void *stream);
/* host pointers: BWT (n bytes) goes up, T_out (n bytes) comes back */
int32_t sa_amd_unbwt(const uint8_t *BWT, int32_t n, int32_t primary, uint8_t *T_out);

typedef struct sa_amd_unbwt_stats {  /* of the calling thread's most recent inverse transform */
    int64_t walkers;                 /* splitters = lanes of a walk launch (the last attempt's) */
    int64_t steps;                   /* psi steps taken by all walkers, both walking phases and every attempt: 2 (n + 1) without a restart */
    int64_t longest_walk;            /* rows of the longest sublist (summed over resumed launches) */
    int32_t splitter_spacing;        /* S in use at the end */
    int32_t walk_launches;           /* launches of the first walking phase, every attempt */
    int32_t restarts;                /* attempts thrown away: lanes were still walking at the launch limit (S / 8, another hash seed) */
    int32_t readbacks;               /* blocking device -> host read-backs of counters */
} sa_amd_unbwt_stats;
void sa_amd_last_unbwt_stats(sa_amd_unbwt_stats *out);
/* route switch of the calling thread's later inverse transforms (never changes a result; there so that the resume and restart
 * paths can be exercised on small inputs).  cap_steps: psi steps one lane takes per walk launch before it saves its place and
 * goes on in the next launch, clamped to 1 .. 16 777 216 (default 4096).  max_launches: walk launches after which an attempt
 * whose lanes are still walking is restarted with denser splitters (default: as many as 64 S steps take; never at S = 4, the
 * densest set).  A negative argument restores that default. */
void sa_amd_unbwt_set_walk_limits(int32_t cap_steps, int32_t max_launches);
/* the same kind of switch for the splitter spacing S of the first attempt: rounded down to a power of two in 4 .. 65 536 (default
 * 256, measured in DESIGN.md section 12); a negative value restores the default.  Returns the previous value. */
int32_t sa_amd_unbwt_set_splitter_spacing(int32_t spacing);

/*
 * Repeat finding (an extension): the longest-repeat array and the byte ranges that are copies, from the text and its suffix
 * array, on the device.  T has n bytes; SA and LCP are in the layout of sa_amd_saca_u8 / sa_amd_lcp
 * (n + 1 entries each); read LCP[n + 1] as 0.
 *   LR (n entries, text order): LR[p] = length of the longest substring starting at p that also starts at some other position
 *     q != p.  Equivalently LR[SA[i]] = max(LCP[i], LCP[i + 1]) for 1 <= i <= n.  p + LR[p] <= n, and LR[p] >= LR[p - 1] - 1:
 *     p + LR[p] never decreases.  "banana": LR = {0, 3, 2, 3, 2, 1}.
 *   Spans, mode SA_AMD_REPEATS_ALL, min_len = k >= 1: the union of [p, p + LR[p]) over all p with LR[p] >= k, as maximal
 *     intervals [start, end), ascending, disjoint and not adjacent: every byte inside some occurrence of a substring of length
 *     >= k that occurs at least twice, first occurrences included.  "banana", k = 2: {[1, 6)}.
 *   Spans, mode SA_AMD_REPEATS_KEEP_FIRST: p is flagged iff the window T[p .. p + k) equals an earlier window T[q .. q + k),
 *     q < p; the spans are the union of [p, p + k) over the flagged p, in the same form.  Equivalently: of every maximal slot
 *     run [a, b] with LCP[a + 1 .. b] >= k all members but the one with the smallest SA value are flagged.  The first copy of
 *     every repeated window survives: what a deduplicator removes.  "banana", k = 2: {[3, 6)}.
 *   A span has at least k bytes and spans are not adjacent: there are at most (n + 1) / (k + 1) of them
 *     (sa_amd_repeat_spans_bound).
 * Spans come as pairs of uint32 (start, end).  `capacity` pairs fit the output: more spans than that is no error -- the first
 * `capacity` are written, *count_out is the number of all of them and the statistics cover all of them.
 * Errors, as for the LCP array: an entry > n is SA_AMD_ERANGE, SA[0] != n is SA_AMD_EINVAL (range pass before anything is read
 * through the entries); min_len < 1, an unknown mode, a negative capacity or a misaligned or short work block is
 * SA_AMD_EINVAL with nothing written.  n = 0: no spans, an empty LR, all-zero statistics (longest_pos -1); n = 1: LR = {0}.
 * The array is not otherwise proved to be the suffix array: with a wrong permutation the answers are unspecified, but nothing
 * is read outside T or the tables and nothing is written outside the outputs.
 */
#define SA_AMD_REPEATS_ALL        0
#define SA_AMD_REPEATS_KEEP_FIRST 1
/* bytes of device scratch the two device calls need: sa_amd_lcp_work_bytes(n) plus one n-entry buffer, about 24.5 (n + 1) */
int64_t sa_amd_repeats_work_bytes(int32_t n);
/* (n + 1) / (min_len + 1); -1 when n < 0 or min_len < 1 */
int64_t sa_amd_repeat_spans_bound(int32_t n, int32_t min_len);
/* device pointers: dT n bytes (any byte address), dSA n + 1 entries, dLR n entries, dWork sa_amd_repeats_work_bytes(n) bytes
 * 256-byte aligned; stream a hipStream_t (NULL = default stream).  Blocks until done. */
int32_t sa_amd_repeat_lengths_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dLR, void *dWork,
                                     int64_t work_bytes, void *stream);
/* dSpans: 2 * capacity entries of device memory (may be NULL when capacity is 0); count_out a HOST pointer */
int32_t sa_amd_repeat_spans_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, int32_t min_len, int32_t mode,
                                   uint32_t *dSpans, int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes,
                                   void *stream);
/* host pointers.  SA == NULL: the array is built on the device, used there and never downloaded: n bytes go up, 4 n bytes (LR)
 * or 8 bytes per span come back.  SA != NULL (n + 1 entries): the caller's array goes up instead of being rebuilt. */
int32_t sa_amd_repeat_lengths(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *LR);
int32_t sa_amd_repeat_spans(const uint8_t *T, int32_t n, const uint32_t *SA, int32_t min_len, int32_t mode, uint32_t *spans,
                            int64_t capacity, int64_t *count_out);
/* from the index's resident text and suffix array */
int32_t sa_amd_index_repeat_lengths(const sa_amd_index *ix, uint32_t *LR);
int32_t sa_amd_index_repeat_spans(const sa_amd_index *ix, int32_t min_len, int32_t mode, uint32_t *spans, int64_t capacity,
                                  int64_t *count_out);

typedef struct sa_amd_repeat_stats { /* of the calling thread's most recent repeat call (sa_amd_last_lcp_stats is filled too) */
    int64_t longest;                 /* max LCP = max LR */
    int64_t longest_pos;             /* the smallest p with LR[p] == longest; -1 when longest is 0 */
    int64_t lcp_sum;                 /* sum of the LCP array */
    int64_t distinct_substrings;     /* n (n + 1) / 2 - lcp_sum: the number of distinct non-empty substrings of T */
    int64_t spans;                   /* all spans, written or not (0 after a call that only made LR, as the next two) */
    int64_t covered_bytes;           /* bytes inside the spans */
    int64_t flagged;                 /* positions with LR >= min_len (ALL) or flagged as later copies (KEEP_FIRST) */
    int32_t readbacks, reserved;     /* blocking device -> host read-backs of counters */
} sa_amd_repeat_stats;
void sa_amd_last_repeat_stats(sa_amd_repeat_stats *out);

/*
 * Lempel-Ziv factorisation (an extension): the longest-previous-factor array with a source for every position, and the greedy
 * LZ77 parse that follows from it, from the text and its suffix array, on the device.  T has n bytes;
 * SA is in the layout of sa_amd_saca_u8 (n + 1 entries, SA[0] = n); "slot" means an index into SA[1 .. n].
 *   For position p with slot i (SA[i] = p): P(p) = SA[j] for the nearest slot j < i with SA[j] < p, N(p) = SA[k] for the nearest
 *     slot k > i with SA[k] < p (n where there is none); lp(p) = lcp(T[p..], T[P(p)..]) (0 when P(p) = n), ln(p) likewise.
 *   LPF (n entries, text order): LPF[p] = max(lp(p), ln(p)) = the length of the longest prefix of T[p..] that also starts at
 *     some q < p (the copy may overlap p).  LPF[p] >= LPF[p - 1] - 1.
 *   SRC (n entries): P(p) if lp(p) >= ln(p) and LPF[p] > 0; N(p) if ln(p) > lp(p); SA_AMD_LZ_LITERAL if LPF[p] = 0.
 *     "banana": LPF = {0, 0, 0, 3, 2, 1}, SRC = {LIT, LIT, LIT, 1, 2, 3} (position 5 has no smaller left neighbour; the right one is 3).
 *   Parse: phrase starts s_0 = 0, s_{k+1} = s_k + max(1, LPF[s_k]) until n is reached; phrase k is the pair of uint32
 *     (SRC[s_k], max(1, LPF[s_k])), a literal (SA_AMD_LZ_LITERAL, 1): the byte T[s_k] itself.  The lengths sum to n; there are
 *     at most n phrases and none for n = 0.  "banana": {(LIT, 1), (LIT, 1), (LIT, 1), (1, 3)}.
 * `capacity` pairs fit the output: more phrases than that is no error -- the first `capacity` are written, *count_out is the
 * number of all of them and the statistics cover all of them.
 * Errors, as for the LCP array: an entry > n is SA_AMD_ERANGE, SA[0] != n is SA_AMD_EINVAL (range pass before anything is read
 * through the entries); a negative capacity or a misaligned or short work block is SA_AMD_EINVAL with nothing written.
 * The array is not otherwise proved to be the suffix array: with a wrong permutation the answers are unspecified, but nothing
 * is read outside T or the tables, nothing is written outside the outputs and every walk terminates.
 */
#define SA_AMD_LZ_LITERAL 0xffffffffu
/* bytes of device scratch the two device calls need: sa_amd_lcp_work_bytes(n) plus three n-entry buffers, about 32 (n + 1) */
int64_t sa_amd_lz_work_bytes(int32_t n);
/* device pointers: dT n bytes (any byte address), dSA n + 1 entries, dLPF and dSRC n entries each (either may be NULL), dWork
 * sa_amd_lz_work_bytes(n) bytes 256-byte aligned; stream a hipStream_t (NULL = default stream).  Blocks until done. */
int32_t sa_amd_lpf_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dLPF, uint32_t *dSRC, void *dWork,
                          int64_t work_bytes, void *stream);
/* dPhrases: 2 * capacity entries of device memory (may be NULL when capacity is 0); count_out a HOST pointer */
int32_t sa_amd_lz77_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, uint32_t *dPhrases, int64_t capacity,
                           int64_t *count_out, void *dWork, int64_t work_bytes, void *stream);
/* host pointers.  SA == NULL: the array is built on the device, used there and never downloaded: n bytes go up, 4 n bytes per
 * array (LPF, SRC; either may be NULL) or 8 bytes per phrase come back.  SA != NULL (n + 1 entries): the caller's array goes up. */
int32_t sa_amd_lpf(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *LPF, uint32_t *SRC);
int32_t sa_amd_lz77(const uint8_t *T, int32_t n, const uint32_t *SA, uint32_t *phrases, int64_t capacity, int64_t *count_out);
/* from the index's resident text and suffix array */
int32_t sa_amd_index_lpf(const sa_amd_index *ix, uint32_t *LPF, uint32_t *SRC);
int32_t sa_amd_index_lz77(const sa_amd_index *ix, uint32_t *phrases, int64_t capacity, int64_t *count_out);

typedef struct sa_amd_lz_stats {     /* of the calling thread's most recent LPF / LZ77 call (sa_amd_last_lcp_stats is filled too:
                                        irreducible positions and compared bytes of both value passes together) */
    int64_t phrases;                 /* all phrases, written or not (0 after a call that only made LPF / SRC, as the next three) */
    int64_t literals;                /* phrases that are a literal byte */
    int64_t longest;                 /* length of the longest phrase */
    int64_t longest_pos;             /* where the first phrase of that length starts; -1 when there is no phrase */
    int64_t unresolved;              /* slots whose nearest smaller value, on either side, was not inside their tile of 1024 slots */
    int64_t hierarchy_steps;         /* words of the block minima (and of SA) those slots loaded, all of them together */
    int64_t hierarchy_max;           /* the most one side of one slot loaded: at most 31 (K - 1) + 32 K, K the number of levels */
    int64_t walkers;                 /* splitters = lanes of a walk launch (the last attempt's) */
    int64_t walk_steps;              /* steps of all walkers, both walking phases and every attempt */
    int32_t walk_launches;           /* launches of the first walking phase, every attempt */
    int32_t restarts;                /* attempts thrown away: lanes were still walking at the launch limit (S / 8, another hash seed) */
    int32_t splitter_spacing;        /* S in use at the end (0 after a call that only made LPF / SRC) */
    int32_t readbacks;               /* blocking device -> host read-backs of counters */
} sa_amd_lz_stats;
void sa_amd_last_lz_stats(sa_amd_lz_stats *out);
/* The parse's walk takes its route switches from sa_amd_unbwt_set_walk_limits and sa_amd_unbwt_set_splitter_spacing (the code
 * is shared); they never change a result. */

/*
 * Matching a query text against the index (an extension): matching statistics and the spans of the query that occur in the
 * indexed text, on the device.  The index text T has n bytes and SA is in the layout of sa_amd_saca_u8;
 * the query Q has m bytes and the cap is C = max_len >= 1.
 *   For query position j the window is w = Q[j .. j + c), c = min(C, m - j).  Let i be the number of slots of SA[0 .. n] whose
 *     suffix is smaller than w in slice order (the lower bound; 1 <= i <= n + 1), a = lcp(w, T[SA[i - 1] ..]) and
 *     b = lcp(w, T[SA[i] ..]) when i <= n, else b = -1.
 *   ML (m entries): ML[j] = max(a, b): the length, capped at C, of the longest prefix of Q[j ..] that occurs in T.
 *   POS (m entries): SA[i - 1] if a > b, else SA[i]; SA_AMD_MATCH_NONE when ML[j] = 0.  T[POS[j] .. POS[j] + ML[j]) equals
 *     Q[j .. j + ML[j]).  For n = 0 every ML is 0.  ML[j + 1] >= ML[j] - 1 when no window is cut by C.
 *     T = "banana", Q = "bandana", C = 8: ML = {3, 2, 1, 0, 3, 2, 1}, POS = {0, 1, 2, NONE, 3, 4, 5}.
 *   Where ML[j] > 0 this is what sa_amd_index_search reports as lcp_len / lcp_start for the pattern w on an index WITHOUT a
 *     bucket table.  The answers here do not depend on whether the index has a bucket table or an LCP table: the rule by which
 *     sa_amd_index_search answers from the top-level bucket when the pattern's bucket is empty does not apply -- the insertion
 *     point is the same with and without the table, and its two neighbours are compared.
 *   Shared spans, min_len = k >= 1: position j is flagged iff m - j >= k and Q[j .. j + k) occurs in T (ML[j] = k under cap k);
 *     the spans are the union of [j, j + k) over the flagged j, as maximal intervals [start, end) in Q: ascending, disjoint and
 *     not adjacent, pairs of uint32.  The same union as that of [j, j + ML'[j]) over all j with uncapped ML'[j] >= k.  At most
 *     (m + 1) / (k + 1) spans (sa_amd_repeat_spans_bound(m, k)); `capacity` / *count_out as for sa_amd_repeat_spans: more spans
 *     than fit is no error, the first `capacity` are written, *count_out and the statistics cover all of them.
 * Errors, each with nothing written: a NULL index, m < 0, a NULL query with m > 0, max_len / min_len < 1, a negative capacity, a
 * misaligned or short work block: SA_AMD_EINVAL.  If the resident array is not the suffix array of the text the answers are
 * unspecified, but nothing is read outside T, Q or the tables and nothing is written outside the outputs.
 * Cost: a position whose compares stay below the group cap (sa_amd_match_set_group_cap) loads at most
 * (ceil(log2(n + 1)) + 3) (min(c, cap) + 4 G) text bytes, G the lanes of a group; the others take one wave each: at most
 * 2 c + 128 log2 P bytes over the LCP table (after sa_amd_index_enable_lcp), else (ceil(log2(n + 1)) + 3) (c + 64) -- O(c log n).
 */
#define SA_AMD_MATCH_NONE 0xffffffffu
/* bytes of device scratch the two device calls need for a query of m bytes: about 5 m */
int64_t sa_amd_match_work_bytes(int32_t m);
/* host pointers: Q goes up, ML and POS (m entries each; either may be NULL) come back */
int32_t sa_amd_index_match_stats(const sa_amd_index *ix, const uint8_t *Q, int32_t m, int32_t max_len, uint32_t *ML, uint32_t *POS);
/* device pointers on the index's device: dQ m bytes (any byte address), dML and dPOS m entries each (either may be NULL), dWork
 * sa_amd_match_work_bytes(m) bytes 256-byte aligned; stream a hipStream_t (NULL = default stream).  Blocks until done. */
int32_t sa_amd_index_match_stats_device(const sa_amd_index *ix, const uint8_t *dQ, int32_t m, int32_t max_len, uint32_t *dML,
                                        uint32_t *dPOS, void *dWork, int64_t work_bytes, void *stream);
/* host pointers: Q goes up, only the spans (8 bytes each) and the counters come back */
int32_t sa_amd_index_match_spans(const sa_amd_index *ix, const uint8_t *Q, int32_t m, int32_t min_len, uint32_t *spans,
                                 int64_t capacity, int64_t *count_out);
/* dSpans: 2 * capacity entries of device memory (may be NULL when capacity is 0); count_out a HOST pointer */
int32_t sa_amd_index_match_spans_device(const sa_amd_index *ix, const uint8_t *dQ, int32_t m, int32_t min_len, uint32_t *dSpans,
                                        int64_t capacity, int64_t *count_out, void *dWork, int64_t work_bytes, void *stream);

typedef struct sa_amd_match_stats {  /* of the calling thread's most recent match call */
    int64_t positions;               /* m */
    int64_t matched;                 /* positions with ML > 0 */
    int64_t longest;                 /* max ML */
    int64_t longest_pos;             /* the first j with ML[j] == longest; -1 when there is none */
    int64_t ml_sum;                  /* sum of ML */
    int64_t long_positions;          /* positions that left the group path: c > cap and ML >= cap */
    int64_t compared_bytes;          /* text bytes loaded for comparison, every chunk (4 G bytes of a group, 64 of a wave) counted whole */
    int64_t steps;                   /* suffixes probed (table steps of the LCP route included) */
    int64_t spans;                   /* all spans, written or not (0 after a stats call, as the next two) */
    int64_t covered_bytes;           /* query bytes inside the spans */
    int64_t flagged;                 /* flagged positions */
    int32_t route_long;              /* route of the long positions: 0 plain wave search, 1 LCP table */
    int32_t readbacks;               /* blocking device -> host read-backs of counters */
    int32_t group_lanes;             /* G */
    int32_t group_cap;               /* the cap in effect: min(sa_amd_match_set_group_cap, 4096 -- what a workgroup stages) */
    int32_t tile;                    /* query positions per workgroup */
    int32_t reserved;
} sa_amd_match_stats;
void sa_amd_last_match_stats(sa_amd_match_stats *out);
/* route switch of the calling thread's later match calls (never changes a result): bytes of a window a group compares before the
 * position goes to the one-wave-per-position path, clamped to 0 .. 1 048 576 (0: every position takes it; above 4096 acts as
 * 4096); a negative value restores the default (64).  Returns the previous value. */
int32_t sa_amd_match_set_group_cap(int32_t bytes);
/* the same kind of switch for G, the lanes that serve one position on the group path: rounded down to 4, 8 or 16 (default 8); a
 * negative value restores the default.  Returns the previous value. */
int32_t sa_amd_match_set_group_lanes(int32_t lanes);

/*
 * Document collections over the index (an extension): which document a position lies in, in how many documents a pattern
 * occurs and in which ones, on the device.  The index text T has n bytes and SA is in the layout of
 * sa_amd_saca_u8.
 *   A collection is doc_off[0 .. ndocs], uint32: ndocs >= 1, doc_off[0] = 0, doc_off[ndocs] = n, non-decreasing -- empty documents
 *     are legal anywhere, and so is an empty text with ndocs empty documents.  Document d is the byte range
 *     [doc_off[d], doc_off[d + 1]).
 *   doc(p), 0 <= p < n, is the unique d with doc_off[d] <= p < doc_off[d + 1]; for p >= n it is SA_AMD_DOC_NONE.  That covers
 *     SA_AMD_MATCH_NONE: a POS array of sa_amd_index_match_stats can be passed straight to sa_amd_index_doc_of.
 *   An occurrence of a pattern belongs to the document in which it STARTS.  A pattern can match across a boundary of the
 *     concatenation; a caller who does not want that separates the documents by a byte their patterns do not contain.
 *   For a pattern whose matches are the slots [lo, hi) -- exactly the range sa_amd_index_search reports --:
 *     occ = hi - lo;
 *     df = the number of distinct doc(SA[i]) over lo <= i < hi with SA[i] < n.  The empty suffix belongs to no document: the
 *       empty pattern has occ = n + 1 and df = the number of non-empty documents;
 *     the listing is those distinct documents, each once, in the order of the slot of their first occurrence in the range
 *       (ordered by each document's lexicographically smallest matching suffix): deterministic, and it costs no sort.
 *     T = "abracadabra", doc_off = {0, 4, 4, 7, 11} (documents "abra", "", "cad", "abra"): "a" has occ 5, df 3 and the listing
 *       {3, 0, 2} (its slots hold the suffixes 10, 7, 0, 3, 5); "bra" has occ 2, df 2, listing {3, 0}; "" has df 3.
 * sa_amd_index_set_documents checks doc_off on the host, uploads it and keeps ONE uint32 per slot next to the offsets
 * (4 (n + 1) bytes): the previous slot of the same document + 1, 0 where there is none, 0xffffffff in slot 0 -- so "first of its
 * document inside [lo, hi)" is the one compare `word <= lo`.  Calling it again replaces the collection; on any failure the
 * previous collection stays.  Not to be called while another thread queries the index; queries may run concurrently.
 * Errors, each with nothing written: a NULL index, a query before sa_amd_index_set_documents, a negative count or capacity,
 * pat_off as sa_amd_index_search rejects it, a malformed doc_off, a device pointer of sa_amd_index_doc_of_device that is not
 * 4-byte aligned: SA_AMD_EINVAL.  If the resident array is not the suffix array of the text the answers are unspecified, but
 * nothing is read outside the tables and nothing is written outside the outputs.
 * Cost: set_documents is one binary search per slot and one stable LSD sort of n pairs over the bits ndocs needs; a query
 * streams 4 bytes per occurrence (twice for a listing) and does one binary search per listed document: O(occ), not O(df).
 */
#define SA_AMD_DOC_NONE 0xffffffffu
/* bytes of device scratch sa_amd_index_set_documents takes from the pool for a text of n bytes: about 16 n */
int64_t sa_amd_docs_work_bytes(int32_t n);
int32_t sa_amd_index_set_documents(sa_amd_index *ix, const uint32_t *doc_off, int64_t ndocs);
/* host pointers: pos (count entries, any values) goes up, doc(pos[i]) comes back */
int32_t sa_amd_index_doc_of(const sa_amd_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out);
/* device pointers on the index's device, 4-byte aligned, count entries each; the call needs no scratch; stream a hipStream_t
 * (NULL = default stream).  Blocks until done. */
int32_t sa_amd_index_doc_of_device(const sa_amd_index *ix, const uint32_t *dPos, int64_t count, uint32_t *dDoc, void *stream);
/* patterns as for sa_amd_index_search; occ and df: count entries each, either may be NULL */
int32_t sa_amd_index_doc_search(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, uint32_t *occ,
                                uint32_t *df);
/* the listing of pattern q is docs[list_off[q] .. list_off[q + 1]) (list_off: count + 1 entries).  More entries than fit is no
 * error: the first `capacity` are written, *total_out (= list_off[count]) and list_off describe all of them. */
int32_t sa_amd_index_doc_list(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int64_t *list_off,
                              uint32_t *docs, int64_t capacity, int64_t *total_out);

typedef struct sa_amd_docs_stats {   /* of the calling thread's most recent doc_search / doc_list call */
    int64_t patterns;
    int64_t occ_sum;                 /* sum of occ */
    int64_t units;                   /* pieces of at most `chunk` slots the ranges were cut into, one wave each */
    int64_t df_sum;                  /* sum of df = entries of the whole listing */
    int64_t slots_scanned;           /* per-slot words streamed: occ_sum for doc_search, twice that for doc_list */
    int32_t chunk;                   /* slots per unit in effect */
    int32_t readbacks;               /* blocking device -> host read-backs of counters: 1 (the number of units) */
    int32_t listed;                  /* 1 after doc_list, 0 after doc_search */
    int32_t reserved;
} sa_amd_docs_stats;
void sa_amd_last_docs_stats(sa_amd_docs_stats *out);
/* route switch of the calling thread's later doc_search / doc_list calls (never changes a result): slots per unit, clamped to
 * 64 .. 1 048 576; a negative value restores the default (4096).  Returns the previous value. */
int32_t sa_amd_docs_set_chunk(int32_t slots);

/*
 * Document-aware duplicate spans (an extension): the byte ranges that are copies, with the document boundaries of the
 * collection respected, and how many bytes of every document they cover, on the device.  T has n bytes,
 * SA is in the layout of sa_amd_saca_u8, the collection is doc_off[0 .. ndocs] as sa_amd_index_set_documents took it and
 * min_len = k >= 1.  Write ds(p) = doc_off[doc(p)] and de(p) = doc_off[doc(p) + 1].
 *   Window and member: the window of p is T[p .. p + k).  p is a MEMBER iff the window lies inside its document:
 *     p + k <= de(p).  A window cut by a document end does not exist here: it is never flagged and never serves as somebody's copy.
 *   Scope SA_AMD_DOCREP_ANY: another member q != p with the same window, in any document.
 *   Scope SA_AMD_DOCREP_OTHER: such a q with doc(q) != doc(p).
 *   Mode SA_AMD_REPEATS_ALL: p is flagged iff such a q exists.
 *   Mode SA_AMD_REPEATS_KEEP_FIRST: p is flagged iff such a q exists with q < p.  Under OTHER this is the same as
 *     doc(q) < doc(p), because documents are ordered by position: the first copy survives, under OTHER the copy in the first
 *     document that has it.
 *   Equivalently, over the maximal slot runs [a, b] with LCP[a + 1 .. b] >= k (those of sa_amd_repeat_spans' KEEP_FIRST):
 *     non-members are transparent -- they break no run and contribute nothing --; with mn / mx the smallest / largest member
 *     position of the run, a member p is flagged iff
 *                      ANY                    OTHER
 *       KEEP_FIRST     mn < p                 mn < ds(p)
 *       ALL            mn < p or mx > p       mn < ds(p) or mx >= de(p)
 *   Spans: the union of [p, p + k) over the flagged p, as maximal intervals [start, end): ascending, disjoint, not adjacent,
 *     pairs of uint32 -- the form of sa_amd_repeat_spans; at most sa_amd_repeat_spans_bound(n, k) of them.  Every covered byte
 *     lies in a window inside its own document, but two spans that touch a document boundary from both sides merge into one:
 *     spans are not split at boundaries, doc_bytes carries the per-document accounting.
 *   doc_bytes[d] (ndocs entries, optional): the covered bytes inside document d; they sum to covered_bytes.
 *   "abracadabra", doc_off = {0, 4, 4, 7, 11}: KEEP_FIRST, ANY, k = 1 flags {3, 5, 7, 8, 9, 10}: spans {[3,4), [5,6), [7,11)};
 *     KEEP_FIRST, OTHER, k = 1 flags {5, 7, 8, 9, 10} (the 'a' at 3 has its first copy in its own document):
 *     doc_bytes = {0, 0, 1, 4}; ALL, k = 3, either scope, flags {0, 1, 7, 8}.
 *   "aaaa", doc_off = {0, 2, 4}, k = 2 (the members are 0 and 2): KEEP_FIRST gives {[2, 4)} where the boundary-blind
 *     sa_amd_repeat_spans gives {[1, 4)}; ALL gives the single span {[0, 4)}, merged across the boundary, doc_bytes = {2, 2}.
 *   With ndocs = 1: scope ANY gives exactly the spans, span count, flagged count and covered bytes of
 *     sa_amd_index_repeat_spans for the same mode (for ALL the union of the k-windows equals the union of the
 *     [p, p + LR[p]), since LR[p + 1] >= LR[p] - 1); scope OTHER gives nothing.
 * `capacity` / *count_out as for sa_amd_repeat_spans: more spans than fit is no error, the first `capacity` are written,
 * *count_out and the statistics cover all of them.
 * Errors, each with nothing written: a NULL index, no collection set, min_len < 1, an unknown mode or scope, a negative
 * capacity, a NULL count_out, capacity > 0 with NULL spans: SA_AMD_EINVAL.  The array's range errors are those of
 * sa_amd_index_repeat_spans.  With a wrong permutation the answers are unspecified, but nothing is read outside the tables and
 * nothing is written outside the outputs.  Every position is below n + 1 < 2^31 and every sum with min_len is taken in 64 bits.
 * sa_amd_last_repeat_stats and sa_amd_last_lcp_stats are filled as by sa_amd_index_repeat_spans (the LCP front end runs).
 * Cost: the LCP front end, one search of doc_off per slot (a sampled level in LDS, then a few loads), and passes that stream
 * 12 to 16 bytes per slot.
 */
#define SA_AMD_DOCREP_ANY   0
#define SA_AMD_DOCREP_OTHER 1
/* bytes of device scratch the call takes from the pool: sa_amd_repeats_work_bytes(n) plus 4 bytes per document; -1 when n < 0
 * or ndocs < 1 */
int64_t sa_amd_doc_repeats_work_bytes(int32_t n, int64_t ndocs);
/* host pointers: only the spans (8 bytes each), doc_bytes (ndocs entries, or NULL: the accounting pass does not run) and the
 * counters come back */
int32_t sa_amd_index_doc_repeat_spans(const sa_amd_index *ix, int32_t min_len, int32_t mode, int32_t scope, uint32_t *spans,
                                      int64_t capacity, int64_t *count_out, uint32_t *doc_bytes);

typedef struct sa_amd_doc_repeat_stats { /* of the calling thread's most recent sa_amd_index_doc_repeat_spans */
    int64_t members;                 /* positions whose window lies inside their document */
    int64_t flagged;                 /* flagged positions */
    int64_t spans;                   /* all spans, written or not */
    int64_t covered_bytes;           /* bytes inside the spans */
    int64_t docs_touched;            /* documents with at least one covered byte; -1 when doc_bytes was NULL (no accounting pass) */
    int32_t readbacks, reserved;     /* blocking device -> host read-backs of counters: the front end's and one more */
} sa_amd_doc_repeat_stats;
void sa_amd_last_doc_repeat_stats(sa_amd_doc_repeat_stats *out);

/*
 * Per-document term frequencies and top-k documents (an extension): how often a pattern occurs in each document it occurs in,
 * and the k documents that hold most of its occurrences, on the device.  The collection is
 * doc_off[0 .. ndocs] as sa_amd_index_set_documents took it; a pattern's matches are the slots [lo, hi) that
 * sa_amd_index_search reports; an occurrence belongs to the document it starts in.
 *   Term frequency: tf(d) = the number of slots i in [lo, hi) with SA[i] < n and doc(SA[i]) = d.  The sum of tf over the listing
 *     equals occ -- less one for the empty pattern, because slot 0 belongs to no document.  For the empty pattern tf(d) is
 *     the length of document d.
 *   sa_amd_index_doc_tf returns the listing of sa_amd_index_doc_list -- the same documents, in the same first-slot order, with
 *     the same list_off -- and a tf entry next to every document.
 *   sa_amd_index_doc_topk takes 1 <= k <= SA_AMD_DOC_TOPK_MAX and returns, per pattern, the min(k, df) documents with the
 *     greatest tf, ordered by tf descending and then by document id ascending.  Entry t of pattern q stands at top_off[q] + t;
 *     top_off[count] is the sum of min(k, df).  The order on (tf descending, id ascending) is strict: the answer is unique.
 *   T = "abracadabra", doc_off = {0, 4, 4, 7, 11}: "a" has the listing {3, 0, 2} with tf {2, 2, 1}; its top-1 is (0, 2), its
 *     top-2 is (0, 2), (3, 2), its top-5 is (0, 2), (3, 2), (2, 1).  "bra" has tf {1, 1}.  "" has the listing {3, 0, 2} with
 *     tf {4, 4, 3}.
 * sa_amd_index_enable_doc_freq keeps one more uint32 per byte of text in the index (4 n bytes): the array S of the slots 1 .. n
 * ordered by document, ascending inside a document.  Document d owns exactly S[doc_off[d] .. doc_off[d + 1]) -- every position
 * of d has one slot -- so tf(d) = lb(S_d, hi) - lb(S_d, lo), lb the lower bound in S_d.  It is the order the stable sort of
 * sa_amd_index_set_documents produces (same scratch, sa_amd_docs_work_bytes).  A no-op when the table exists; SA_AMD_EINVAL
 * when no collection is set, SA_AMD_ENOMEM when the table does not fit.  sa_amd_index_set_documents drops the table when it
 * replaces the collection: the caller enables it again.  The threading rule of sa_amd_index_set_documents applies.
 * Errors, each with nothing written: a NULL index, no collection, no frequency table, a negative count or capacity, pat_off as
 * sa_amd_index_search rejects it, k outside 1 .. SA_AMD_DOC_TOPK_MAX, a NULL list_off, top_off or total_out: SA_AMD_EINVAL.
 * The downloads into tf and then docs are the last two steps that can fail; list_off / top_off and *total_out are written
 * behind both: a failing call can leave tf (partly) written and everything else untouched.  With an array that is no suffix array the answers are unspecified, but nothing is read outside the tables and nothing
 * is written outside the outputs.
 * Cost: the listing's 2 occ streamed words, O(log |d| + log tf) loads of S per listed document, and for the top-k a sort in
 * LDS of pieces of the listing: pieces of P keys keep their first k, the kept keys are cut into pieces again until every
 * pattern is one piece.
 */
#define SA_AMD_DOC_TOPK_MAX 1024
int32_t sa_amd_index_enable_doc_freq(sa_amd_index *ix);
/* capacity, list_off and *total_out exactly as for sa_amd_index_doc_list: more entries than fit is no error, the first `capacity`
 * entries of docs and of tf are written.  Either of docs and tf may be NULL. */
int32_t sa_amd_index_doc_tf(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int64_t *list_off,
                            uint32_t *docs, uint32_t *tf, int64_t capacity, int64_t *total_out);
/* top_off: count + 1 entries; docs and tf: count * k entries each (a 64-bit product), written compactly up to top_off[count].
 * Either of docs and tf may be NULL. */
int32_t sa_amd_index_doc_topk(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count, int32_t k,
                              int64_t *top_off, uint32_t *docs, uint32_t *tf);

typedef struct sa_amd_doc_tf_stats { /* of the calling thread's most recent doc_tf / doc_topk call (sa_amd_last_docs_stats is not touched) */
    int64_t patterns;
    int64_t occ_sum;                 /* sum of occ */
    int64_t df_sum;                  /* entries of the whole listing */
    int64_t tf_sum;                  /* sum of the tf computed: of the whole listing, or of its first `capacity` entries */
    int64_t table_loads;             /* loads of S, all lanes */
    int64_t topk_entries;            /* top_off[count]; 0 after doc_tf */
    int64_t pieces;                  /* workgroups of all reduction rounds */
    int32_t rounds;                  /* reduction rounds: the last leaves one piece per pattern (at least 1 for a doc_topk with patterns) */
    int32_t k;                       /* 0 after doc_tf */
    int32_t piece;                   /* the effective P; 0 after doc_tf */
    int32_t chunk;                   /* slots per unit of the listing in effect (sa_amd_docs_set_chunk) */
    int32_t readbacks;               /* blocking device -> host read-backs of counters: the listing's and the tf kernel's */
    int32_t reserved;
} sa_amd_doc_tf_stats;
void sa_amd_last_doc_tf_stats(sa_amd_doc_tf_stats *out);
/* route switch of the calling thread's later doc_topk calls (never changes a result): keys per piece P, rounded down to a power
 * of two in 64 .. 4096; a negative value restores the default (1024).  Returns the previous value.  A call raises P to at least
 * twice the next power of two >= k, so that every round at least halves a list longer than P.  sa_amd_docs_set_chunk applies to
 * doc_tf and doc_topk as it does to doc_list. */
int32_t sa_amd_docs_set_topk_piece(int32_t entries);

/*
 * Repeated substrings (an extension): which substrings occur at least twice, how often, and the most frequent, the longest or
 * the most covering of them, on the device.  The table a unigram tokeniser trainer seeds its vocabulary
 * from and a curator lists boilerplate with, without downloading the suffix array or the LCP array.
 * SA and LCP are in the layout of sa_amd_saca_u8 and sa_amd_lcp: n + 1 entries, LCP[0] = LCP[1] = 0.
 *   A slot i with 2 <= i <= n is a REPRESENTATIVE when both hold: d = LCP[i] > 0; the nearest j < i with LCP[j] <= d has
 *     LCP[j] < d.  That j is lo, and lo >= 1.  hi is the nearest j > i with LCP[j] < d, or n + 1 when there is none.
 *   The NODE of a representative is the row (lo, count, depth, parent): lo as above; count = hi - lo, which is at least 2;
 *     depth = d; parent = max(LCP[lo], LCP[hi]), with LCP[n + 1] read as 0.  This gives parent < depth.
 *   Its substring is T[SA[lo] .. SA[lo] + depth), and it occurs at exactly SA[lo .. lo + count).
 *   The nodes are the internal nodes of the suffix tree below the root: there are at most max(n - 1, 0) of them
 *     (sa_amd_substrings_bound); every substring that occurs at least twice, of length L, lies in exactly one node with
 *     parent < L <= depth and has that node's count; for one node every length in (parent, depth] has the same occurrence set,
 *     so a caller can cut the table at any length without another query.
 *   "banana": LCP = {0, 0, 1, 3, 0, 0, 2}; the nodes are (1, 3, 1, 0) "a", (2, 2, 3, 1) "ana" (and "an") and (5, 2, 2, 0) "na"
 *     (and "n"), at the representatives 2, 3 and 6; pos = {5, 3, 4}.
 * Query: min_len >= 1, max_len (0: none, otherwise >= min_len), min_count >= 2, order and k.  A node is SELECTED when
 *   depth >= min_len, (max_len == 0 or parent < max_len) and count >= min_count.  Its effective length is len = depth when
 *   max_len == 0, otherwise min(depth, max_len).
 * Orders: SA_AMD_SUBSTR_ALL returns every selected node by representative slot ascending and ignores k.  The ranked orders
 *   return the best min(k, selected) nodes by a 64-bit key, descending, equal keys by representative slot ascending:
 *   SA_AMD_SUBSTR_BY_COUNT key = count, SA_AMD_SUBSTR_BY_LENGTH key = len, SA_AMD_SUBSTR_BY_COVER key = count * len (uint64).
 *   They require k >= 1.  The order is strict, so the answer is unique.
 * Outputs: rows of 4 uint32 (lo, count, depth, parent); pos (optional, may be NULL): pos[r] = SA[lo_r], where the substring of
 *   row r can be read in the text.  *total is the number of rows the query has: selected, or min(k, selected) for the ranked
 *   orders.  The first min(capacity, *total) rows are written and nothing behind them; more rows than fit is no error.
 * Errors, as for sa_amd_lcp: an entry > n is SA_AMD_ERANGE, SA[0] != n is SA_AMD_EINVAL (range pass before anything is read
 * through the entries).  A query outside the ranges above, an unknown order, capacity < 0, a NULL total, NULL rows with
 * capacity > 0 and a misaligned or short work block are SA_AMD_EINVAL with nothing written; they are answered before a
 * device is looked for.  SA_AMD_ENOMEM as elsewhere.  With an array that is no suffix array the answers are unspecified, but
 * nothing is read outside T or the tables and nothing is written outside the outputs.
 * The LCP array is built inside (sa_amd_lcp_device's stages): sa_amd_last_lcp_stats is filled by that build, as after
 * sa_amd_lcp; sa_amd_last_lz_stats, sa_amd_last_repeat_stats and the other features' statistics are not touched.
 */
#define SA_AMD_SUBSTR_ALL 0
#define SA_AMD_SUBSTR_BY_COUNT 1
#define SA_AMD_SUBSTR_BY_LENGTH 2
#define SA_AMD_SUBSTR_BY_COVER 3
typedef struct sa_amd_substr_query {
    int32_t min_len;                 /* >= 1 */
    int32_t max_len;                 /* 0: no upper limit; otherwise >= min_len */
    int32_t min_count;               /* >= 2 */
    int32_t order;                   /* SA_AMD_SUBSTR_* */
    int64_t k;                       /* ranked orders: >= 1; ignored by SA_AMD_SUBSTR_ALL */
} sa_amd_substr_query;
/* bytes of device scratch the device call needs: sa_amd_lcp_work_bytes(n) plus five n-entry buffers, about 41 (n + 1); -1 when n < 0 */
int64_t sa_amd_substrings_work_bytes(int32_t n);
/* the most rows any query can have: max(n - 1, 0); -1 when n < 0 */
int64_t sa_amd_substrings_bound(int32_t n);
/* device pointers: dT n bytes (any byte address), dSA n + 1 entries, dRows 4 * capacity entries and dPos capacity entries (dRows
 * may be NULL when capacity is 0, dPos whenever it is not wanted), dWork sa_amd_substrings_work_bytes(n) bytes 256-byte aligned;
 * total a HOST pointer; stream a hipStream_t (NULL = default stream).  Blocks until done. */
int32_t sa_amd_substrings_device(const uint8_t *dT, const uint32_t *dSA, int32_t n, const sa_amd_substr_query *query, uint32_t *dRows,
                                 uint32_t *dPos, int64_t capacity, int64_t *total, void *dWork, int64_t work_bytes, void *stream);
/* host pointers.  SA == NULL: the array is built on the device, used there and never downloaded: n bytes go up, 16 (+ 4) bytes
 * per row come back.  SA != NULL (n + 1 entries): the caller's array goes up. */
int32_t sa_amd_substrings(const uint8_t *T, int32_t n, const uint32_t *SA, const sa_amd_substr_query *query, uint32_t *rows,
                          uint32_t *pos, int64_t capacity, int64_t *total);
/* from the index's resident text and suffix array (with or without sa_amd_index_enable_lcp: its table is not the LCP array) */
int32_t sa_amd_index_substrings(const sa_amd_index *ix, const sa_amd_substr_query *query, uint32_t *rows, uint32_t *pos,
                                int64_t capacity, int64_t *total);

typedef struct sa_amd_substr_stats { /* of the calling thread's most recent substrings call */
    int64_t nodes;                   /* all nodes, whatever the query */
    int64_t selected;                /* nodes the filter keeps, whatever k and capacity */
    int64_t distinct_all;            /* sum of depth - parent over all nodes: the distinct substrings that occur at least twice */
    int64_t distinct_selected;       /* sum of len - max(parent, min_len - 1) over the selected nodes: the distinct substrings
                                        with a length in the window and at least min_count occurrences */
    int64_t unresolved;              /* slots whose neighbour, on either side, was not inside their tile of 1024 slots */
    int64_t far_steps;               /* words of the block minima (and of LCP) those slots loaded, all of them together */
    int64_t far_max;                 /* the most one side of one slot loaded: at most 31 (K - 1) + 32 K, K the number of levels (347) */
    int64_t sorted;                  /* pairs the final sort of a ranked order ran on: min(k, selected); 0 for SA_AMD_SUBSTR_ALL */
    int32_t select_passes;           /* digit histograms of the radix select: at most 8; 0 when k >= selected */
    int32_t readbacks;               /* blocking device -> host read-backs of counters, the LCP build's included */
} sa_amd_substr_stats;
void sa_amd_last_substr_stats(sa_amd_substr_stats *out);

/*
 * Repeated substrings with their document frequency (an extension): in how many documents of the index's collection every
 * repeated substring occurs, and the nodes filtered and ranked by that number, on the device.  A string
 * that occurs 10 000 times inside one log file and a licence header that occurs once in each of 10 000 files have the same
 * count; their document frequencies are 1 and 10 000.  The collection is doc_off[0 .. ndocs] as sa_amd_index_set_documents took
 * it; slots, LCP and the nodes (lo, count, depth, parent) are exactly those of "Repeated substrings" above.
 *   Document frequency: df(node) = the number of distinct doc(SA[i]) over lo <= i < lo + count.  An occurrence belongs to the
 *     document it starts in, as for sa_amd_index_doc_search.  Nodes have lo >= 1, so slot 0 (the empty suffix, which belongs to
 *     no document) is never inside one.  1 <= df <= min(count, the non-empty documents); with ndocs = 1 every df is 1.
 *   A node's substring may cross a document boundary, as a pattern of sa_amd_index_doc_search may: "ab|cd" and "xab|cd" share
 *     "abcd".  A caller who does not want that separates the documents by a byte that cannot repeat usefully (one separator
 *     byte still forms nodes of depth 1 around it).  Nodes that respect the boundaries are not offered.
 *   How it is computed: with P[i] the previous slot of the document of slot i (the index's per-slot word) and m(i) any slot of
 *     (P[i], i] where LCP has its minimum over (P[i], i], G[m] = the number of i with m(i) = m and E the exclusive running sum
 *     of G (n + 2 entries): df = count - (E[lo + count] - E[lo + 1]).  Any such m gives the same df.
 * Query: min_len, max_len, min_count, order and k as in sa_amd_substr_query, with the same ranges; min_docs >= 1, where 1 means
 *   no document filter.  A node is SELECTED when the filter of "Repeated substrings" holds and df >= min_docs.
 * Orders: SA_AMD_SUBSTR_ALL, _BY_COUNT, _BY_LENGTH and _BY_COVER as above.  SA_AMD_SUBSTR_BY_DOCS: key = df, descending, equal
 *   keys by representative slot ascending; k >= 1.  The order is strict, so the answer is unique.  The longest substring common
 *   to at least m documents is SA_AMD_SUBSTR_BY_LENGTH with min_docs = m and k = 1.
 * Outputs: rows of 4 uint32 as above; df and pos are parallel arrays of one uint32 a row, and either may be NULL.  capacity and
 *   *total as for sa_amd_index_substrings: the first min(capacity, *total) rows are written and nothing behind them.
 *   "abracadabra", doc_off = {0, 4, 4, 7, 11} ("abra", "", "cad", "abra"): the nodes are "a" (count 5, df 3), "abra" (2, 2),
 *     "bra" (2, 2) and "ra" (2, 2).  "aaaa", doc_off = {0, 2, 4}: "a" (4, 2), "aa" (3, 2), "aaa" (2, 1).
 *   With min_docs = 1 and the orders 0 .. 3 the rows, pos and *total are bit for bit those of sa_amd_index_substrings for the same
 *     first five fields; df of a row is the df sa_amd_index_doc_search reports for the pattern T[pos .. pos + depth).
 * Errors, each SA_AMD_EINVAL with nothing written and answered before a device is looked for: a NULL index, no collection set,
 * a query outside its ranges or an order outside 0 .. 4, capacity < 0, a NULL total, NULL rows with capacity > 0.  The array's
 * range errors are those of sa_amd_index_substrings.  With an array that is no suffix array the answers are unspecified, but
 * nothing is read outside the tables and nothing is written outside the outputs.
 * sa_amd_last_lcp_stats is filled as by sa_amd_index_substrings; sa_amd_last_substr_stats and every other feature's statistics
 * are not touched.  The threading rule of sa_amd_index_set_documents applies.
 * Cost: sa_amd_index_substrings plus one range-minimum query per slot over the minima its first stage has built -- at most
 * 93 K + 32 loaded words a query, K the number of levels of minima (K = 6, 590 words, for n < 2^31) --, one atomic per slot or
 * fewer, a scan of n + 2 words and two more loads per node.
 */
#define SA_AMD_SUBSTR_BY_DOCS 4
typedef struct sa_amd_doc_substr_query {
    int32_t min_len;                 /* >= 1 */
    int32_t max_len;                 /* 0: no upper limit; otherwise >= min_len */
    int32_t min_count;               /* >= 2 */
    int32_t order;                   /* SA_AMD_SUBSTR_*, SA_AMD_SUBSTR_BY_DOCS included */
    int64_t k;                       /* ranked orders: >= 1; ignored by SA_AMD_SUBSTR_ALL */
    int64_t min_docs;                /* >= 1; 1: no document filter */
} sa_amd_doc_substr_query;
/* bytes of device scratch the call takes from the pool: sa_amd_substrings_work_bytes(n) plus one buffer of n + 2 entries;
 * -1 when n < 0 */
int64_t sa_amd_doc_substrings_work_bytes(int32_t n);
/* host pointers: 16 (+ 4 + 4) bytes per row come back */
int32_t sa_amd_index_doc_substrings(const sa_amd_index *ix, const sa_amd_doc_substr_query *query, uint32_t *rows, uint32_t *df,
                                    uint32_t *pos, int64_t capacity, int64_t *total);

typedef struct sa_amd_doc_substr_stats { /* of the calling thread's most recent sa_amd_index_doc_substrings */
    int64_t nodes;                   /* all nodes, whatever the query */
    int64_t selected;                /* nodes the filter keeps, df >= min_docs included, whatever k and capacity */
    int64_t distinct_selected;       /* sum of len - max(parent, min_len - 1) over the selected nodes */
    int64_t df_sum;                  /* sum of df over the selected nodes */
    int64_t max_df;                  /* the largest df of a selected node; 0 when none is selected */
    int64_t pairs;                   /* slots that have a previous slot of their document: n less the non-empty documents */
    int64_t rmq_far;                 /* pairs whose range (previous slot, slot] does not lie inside one block of 32 slots */
    int64_t rmq_steps;               /* words of LCP and of its minima the range-minimum queries loaded, all of them together */
    int64_t rmq_max;                 /* the most one query loaded: at most 93 K + 32, K the number of levels of minima */
    int64_t sorted;                  /* pairs the final sort of a ranked order ran on: min(k, selected); 0 for SA_AMD_SUBSTR_ALL */
    int32_t select_passes;           /* digit histograms of the radix select: at most 8; 0 when k >= selected */
    int32_t readbacks;               /* blocking device -> host read-backs of counters, the LCP build's included */
} sa_amd_doc_substr_stats;
void sa_amd_last_doc_substr_stats(sa_amd_doc_substr_stats *out);

/*
 * n-gram and infinity-gram queries (an extension): what follows a context in the text and how often, and the longest suffix
 * of a prompt that occurs often enough, on the device.  T has n bytes, SA has n + 1 slots in the layout
 * of sa_amd_saca_u8; a context c of p bytes has the match range [lo, hi) that sa_amd_index_search reports.
 *   at_end is 1 iff some slot of the range has SA[i] + p == n: the context is a suffix of the text.  It can only be slot lo
 *     (the suffix that is the context itself is the smallest one that starts with it).  Otherwise at_end is 0.
 *   next[b] = the number of slots i in [lo, hi) with SA[i] + p < n and T[SA[i] + p] == b.
 *   sum(next) + at_end == hi - lo.
 *   Inside the range the slots are ordered by the byte behind the context: those with continuation b are the contiguous
 *     sub-range that starts at lo + at_end + sum(next[b'] for b' < b) and has next[b] slots.  It is the range of c + b: a caller
 *     descends from a context to a longer one without another search.
 *   The LISTING of a context is its non-zero (b, next[b]) pairs in ascending b: at most 256 entries.
 *   The empty context has the range [0, n + 1) and at_end = 1; its listing is the byte histogram of T.
 *   A context that does not occur has lo == hi, at_end = 0 and an empty listing.
 * Back-off (sa_amd_index_infgram), for a prompt P of L bytes, min_count >= 1 and max_len:
 *   max_len <= 0 means no cap: cap = L, otherwise cap = min(L, max_len).
 *   s = the largest value in 0 .. cap such that P[L - s .. L) has at least min_count occurrences (hi - lo >= min_count).
 *   s = 0 always qualifies, also when min_count > n + 1: the fallback is the unigram distribution.
 *   The count never grows with s, so s is well defined and found by bisection: at most 2 ceil(log2(cap + 1)) + 2 range
 *     searches per prompt (this implementation runs at most ceil(log2(cap + 1))).
 *   The outputs are s, the range of that suffix, its at_end and its listing.
 *   T = "abracadabra", SA = {11,10,7,0,3,5,8,1,4,6,9,2}:
 *     context   range     at_end  listing
 *     "a"       [1, 6)    1       {b:2, c:1, d:1}
 *     "abra"    [2, 4)    1       {c:1}
 *     ""        [0, 12)   1       {a:5, b:2, c:1, d:1, r:2}
 *     "x"       empty     0       empty
 *     prompt    min_count max_len  s   range
 *     "xcabra"  1         none     4   [2, 4)
 *     "xcabra"  2         none     4   [2, 4)
 *     "xcabra"  3         none     1   [1, 6)   ("a")
 *     "xcabra"  1         2        2   [10, 12) ("ra")
 * Patterns are passed as for sa_amd_index_search.  The listing follows sa_amd_index_doc_tf: list_off has count + 1 entries, the
 * listing of pattern q is (bytes, counts)[list_off[q] .. list_off[q + 1]); more entries than `capacity` is no error: the first
 * `capacity` are written, *total_out (= list_off[count]) and list_off describe all of them.  EVERY output pointer may be NULL;
 * bytes and counts may each be NULL, and with both NULL `capacity` is ignored (nothing is emitted).  count == 0 succeeds with
 * list_off[0] = 0.
 * Errors, each with nothing written: a NULL index, a negative count or capacity, pat_off as sa_amd_index_search rejects it,
 * min_count < 1: SA_AMD_EINVAL.  If the resident array is not the suffix array of the text the answers are unspecified, but
 * nothing is read outside the text, the patterns and the tables: every slot read lies in [0, n + 1), every SA entry is checked
 * against n before T is read through it (an entry with SA[i] + p >= n counts as "at end"), and nothing is written outside the
 * outputs.  The answers are the same with or without the bucket table and the LCP table.
 * Cost: per context the range search; then hi - lo slots streamed (each 4 bytes of SA and one byte of text) when the range
 * has at most `stream cap` slots, else at most 64 + 256 (ceil(log2(cnt + 1)) + 1) slots probed, cnt = hi - lo - at_end.  With
 * bytes or counts asked for, the continuations are computed twice (counted, then emitted in order); the probe counters below
 * are those of the counting pass.
 */
int32_t sa_amd_index_next_bytes(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count,
                                uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end,
                                int64_t *list_off, uint8_t *bytes, uint32_t *counts, int64_t capacity, int64_t *total_out);
int32_t sa_amd_index_infgram(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t count,
                             int32_t min_count, int32_t max_len, uint32_t *suffix_len,
                             uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end,
                             int64_t *list_off, uint8_t *bytes, uint32_t *counts, int64_t capacity, int64_t *total_out);

typedef struct sa_amd_ngram_stats {  /* of the calling thread's most recent next_bytes / infgram call (no other feature's statistics are touched) */
    int64_t patterns;
    int64_t range_searches;          /* infgram: the probes of the bisection, all prompts; next_bytes: one per pattern */
    int64_t compared_bytes;          /* infgram: text bytes the range searches compared; -1 after next_bytes (the search kernels do not count) */
    int64_t stream_slots;            /* slots probed by the streaming route: the sum of cnt over its queries, exactly */
    int64_t search_slots;            /* slots probed by the boundary-search route */
    int64_t stream_queries;          /* queries by route: 0 < cnt <= stream_cap */
    int64_t search_queries;          /*                   cnt > stream_cap */
    int64_t empty_queries;           /*                   cnt == 0: nothing is probed */
    int64_t entries;                 /* entries of the whole listing (= *total_out) */
    int32_t stream_cap;              /* the stream cap in effect */
    int32_t readbacks;               /* blocking device -> host read-backs of counters: 1 */
    int32_t backoff;                 /* 1 after infgram, 0 after next_bytes */
    int32_t passes;                  /* runs of the continuation kernel: 1 (counted only: bytes and counts NULL, or capacity 0), else 2 */
} sa_amd_ngram_stats;
void sa_amd_last_ngram_stats(sa_amd_ngram_stats *out);
/* route switch of the calling thread's later next_bytes / infgram calls (never changes a result): ranges of at most `slots`
 * slots (after the at-end slot is stripped) are streamed, longer ones are searched.  0 makes every non-empty range search, a
 * huge value (clamped to 2^31 - 1) makes every range stream; a negative value restores the default (1024).  Returns the
 * previous value. */
int32_t sa_amd_ngram_set_stream_cap(int32_t slots);

/*
 * Scoring a text under the infinity-gram model (an extension): for every position of a query the back-off of
 * sa_amd_index_infgram and the count of the byte that is really there, on the device.  T has n bytes,
 * SA has n + 1 slots; "range of a string" is the [lo, hi) that sa_amd_index_search reports; at_end and next[b] are those of
 * sa_amd_index_next_bytes.
 *   Q has m bytes.  q_off has ndocs + 1 entries, q_off[0] = 0, non-decreasing, q_off[ndocs] = m: document d is
 *   Q[q_off[d] .. q_off[d + 1]), empty documents are allowed.  q_off == NULL means one document [0, m) (ndocs is ignored).
 * For position j of the document that starts at `start`:
 *   cap_j  = min(j - start, max_len): a context never crosses a document start.
 *   S[j]   = the largest s in 0 .. cap_j such that Q[j - s .. j) has hi - lo >= min_count.  s = 0 always qualifies, with the
 *            range [0, n + 1) and at_end = 1.  It is what sa_amd_index_infgram returns as suffix_len for the prompt
 *            Q[start .. j) with the same min_count and max_len.
 *   LO[j], HI[j], AT_END[j] = that suffix's range and at-end flag, again sa_amd_index_infgram's.
 *   NLO[j] = LO + AT_END + sum(next[b'] for b' < Q[j]),  NHI[j] = NLO + next[Q[j]].
 *   Where NHI > NLO, [NLO, NHI) is the range of Q[j - s .. j]; where the continuation does not occur, NHI == NLO is its
 *   insertion point inside the context's range.
 * The model's probability of Q[j] is (NHI - NLO) / (HI - LO - AT_END); the denominator is 0 when the context occurs only as
 * the text's last bytes.
 *   T = "abracadabra", Q = "xcabra", one document, min_count = 1, max_len = 4:
 *     j  byte  S  [LO, HI)  AT_END  [NLO, NHI)
 *     0  x     0  [0, 12)   1       [12, 12)
 *     1  c     0  [0, 12)   1       [8, 9)
 *     2  a     1  [8, 9)    0       [8, 9)
 *     3  b     2  [8, 9)    0       [8, 8)
 *     4  r     2  [2, 4)    0       [2, 4)
 *     5  a     3  [2, 4)    0       [2, 4)
 *   With min_count = 3, position 5 has S = 0: its context ends in "r", which occurs twice.
 * The length is found by galloping (s = 1, 2, 4, ... clamped to cap_j) and a bisection between the last good and the first
 * bad length: at most 2 ceil(log2(S[j] + 2)) + 2 range searches for position j, whatever the group cap below.
 * EVERY output pointer may be NULL.  m == 0 succeeds.  Errors, each with nothing written: a NULL index, m < 0, min_count < 1,
 * max_len outside 1 .. SA_AMD_SCORE_MAX_CONTEXT, with q_off: ndocs < 0 or offsets that break the rules above: SA_AMD_EINVAL.
 * If the resident array is not the suffix array of the text the answers are unspecified, but the reads obey the rules of
 * sa_amd_index_next_bytes: every slot read lies in [0, n + 1), every SA entry is checked against n in 64 bits before T is
 * read through it, Q is read inside [0, m) only and nothing is written outside the outputs.  The answers are the same with or
 * without the bucket table and the LCP table, and for every group cap.
 */
#define SA_AMD_SCORE_MAX_CONTEXT 4096
int32_t sa_amd_index_infgram_score(const sa_amd_index *ix, const uint8_t *Q, int64_t m, const int64_t *q_off, int64_t ndocs,
                                   int32_t min_count, int32_t max_len, uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END,
                                   uint32_t *NLO, uint32_t *NHI);
/* bytes of work space for the device form below; -1 when m or ndocs is negative */
int64_t sa_amd_score_work_bytes(int64_t m, int64_t ndocs);
/* the same code path on device-resident data: dQ and the outputs live on the index's device (any of the outputs NULL), q_off
 * stays a HOST pointer (it is checked, then copied into the work space), dWork is 256-byte aligned with at least
 * sa_amd_score_work_bytes(m, ndocs) bytes (ndocs = 1 where q_off is NULL).  Blocks until done. */
int32_t sa_amd_index_infgram_score_device(const sa_amd_index *ix, const uint8_t *dQ, int64_t m, const int64_t *q_off, int64_t ndocs,
                                          int32_t min_count, int32_t max_len, uint32_t *dS, uint32_t *dLO, uint32_t *dHI,
                                          uint8_t *dAT_END, uint32_t *dNLO, uint32_t *dNHI, void *dWork, int64_t work_bytes,
                                          void *stream);

typedef struct sa_amd_score_stats {  /* of the calling thread's most recent infgram_score call (no other feature's statistics are touched) */
    int64_t positions;               /* m */
    int64_t documents;               /* ndocs; 1 where q_off is NULL */
    int64_t group_searches;          /* range searches of the group path (8 lanes a position, the context in LDS) */
    int64_t long_searches;           /* range searches of the long path (one wave a position) */
    int64_t next_lookups;            /* slots probed by the two lower bounds on the byte behind the context, all positions */
    int64_t compared_bytes;          /* text bytes the range searches compared, chunks charged whole (32 on the group path, up to 64 on the long path) */
    int64_t long_positions;          /* positions finished by the long path */
    int64_t zero_positions;          /* positions with NHI == NLO */
    int32_t group_cap;               /* the cap in effect: min(group cap, max_len, 4096) */
    int32_t readbacks;               /* blocking device -> host read-backs of counters: 1, or 2 with long positions */
} sa_amd_score_stats;
void sa_amd_last_score_stats(sa_amd_score_stats *out);
/* route switch of the calling thread's later infgram_score calls (never changes a result): context bytes a lane group probes
 * before the position goes to the one-wave-per-position path, 0 .. 1 048 576 (0: every position with a context; above 4096
 * acts as 4096); a negative value restores the default (64).  Returns the previous value.  The same switch applies to the
 * calling thread's sa_amd_tok_index_infgram_score calls (below), where it counts context TOKENS. */
int32_t sa_amd_score_set_group_cap(int32_t bytes);

/*
 * Texts over a 16-bit token alphabet (an extension): the suffix array of a text of tokeniser ids, a device-resident token index
 * and the n-gram / infinity-gram queries on it.  T has n tokens, compared as unsigned 16-bit values; a
 * suffix that is a proper prefix of another sorts first.  SA has n + 1 entries in TOKEN positions, SA[0] = n (the layout of
 * sa_amd_saca_u8 with "byte" replaced by "token").  The raw little-endian bytes of T are NOT a substitute: 0x0100 would sort
 * before 0x0001, matches could start in the middle of a token, and the counts would be next-byte counts.
 * Construction: the big-endian byte image of T (2 n bytes) goes through the byte builder, and an order-preserving compaction
 * keeps the even entries of its array, halved.  Peak device memory of sa_amd_saca_u16: 2 n (T) + 2 n (image) + 4 (2 n + 1) +
 * sa_amd_workspace_bytes(2 n), one pooled block; a block that does not fit is SA_AMD_ENOMEM (no reduced-memory route).
 * sa_amd_last_stats is that of the byte build.
 * n == 0 gives SA = {0}.  n < 0, n > sa_amd_max_tokens_u16(), a NULL SA, or a NULL T with n > 0: SA_AMD_EINVAL.
 */
int32_t sa_amd_max_tokens_u16(void);                                              /* 1073741823 = (2^31 - 1) / 2 */
int32_t sa_amd_saca_u16(const uint16_t *T, uint32_t *SA, int32_t n);              /* host pointers */

/*
 * The token index keeps T (2 n bytes) and the token suffix array (4 (n + 1) bytes) in HBM; the byte image and the byte-level
 * array are scratch of the build.  SA == NULL: the array is built on the device and never downloaded.  A supplied SA (n + 1
 * entries) is range-checked before anything reads through it: an entry above n is SA_AMD_ERANGE, SA[0] != n is SA_AMD_EINVAL;
 * with a wrong but in-range array the answers are unspecified, and nothing is read outside T, the patterns and the array.
 * The queries follow sa_amd_index_search, sa_amd_index_next_bytes and sa_amd_index_infgram (above) with "byte" replaced by
 * "token": lengths, pat_off, suffix_len and max_len are in tokens, pat_data holds the patterns' tokens back to back.
 *   at_end is 1 iff some slot of the range has SA[i] + p == n; it can only be slot lo.
 *   next[t] = the number of slots i in [lo, hi) with SA[i] + p < n and T[SA[i] + p] == t;  sum(next) + at_end == hi - lo.
 *   The slots with continuation t are the contiguous sub-range that starts at lo + at_end + sum(next[t'] for t' < t) and has
 *     next[t] slots.  It is the range of c + t.
 *   The LISTING of a context is its non-zero (t, next[t]) pairs in ascending t: at most min(65 536, hi - lo) entries.
 *   The empty context has the range [0, n + 1) and at_end = 1; its listing is the token histogram of T.
 *   A context that does not occur has lo == hi, at_end = 0 and an empty listing.
 *   Back-off: s = the largest value in 0 .. cap (cap = L, or min(L, max_len) where max_len > 0) such that the last s tokens of
 *     the prompt occur at least min_count times; at most ceil(log2(cap + 1)) range searches per prompt.
 *   T = {256, 1, 256, 1, 2}, SA = {5, 3, 1, 4, 2, 0} (the little-endian byte image gives another order):
 *     context     range     at_end  listing
 *     {256, 1}    [4, 6)    0       {2:1, 256:1}
 *     {1}         [1, 3)    0       {2:1, 256:1}
 *     {2}         [3, 4)    1       empty
 *     {}          [0, 6)    1       {1:2, 2:1, 256:2}
 *     {9}         empty     0       empty
 *     prompt       min_count max_len  s   range
 *     {7, 256, 1}  1         none     2   [4, 6)
 *     {7, 256, 1}  3         none     0   [0, 6)
 *     {7, 256, 1}  2         1        1   [1, 3)
 * list_off has count + 1 entries, the listing of pattern q is (tokens, counts)[list_off[q] .. list_off[q + 1]); more entries
 * than `capacity` is no error: the first `capacity` are written, *total_out (= list_off[count]) and list_off describe all of
 * them.  EVERY output pointer may be NULL; tokens and counts may each be NULL, and with both NULL `capacity` is ignored.
 * count == 0 succeeds with list_off[0] = 0.
 * Errors, each with nothing written: a NULL index, a negative count or capacity, pat_off as sa_amd_index_search rejects it,
 * min_count < 1: SA_AMD_EINVAL.
 * Cost: a search is a plain binary search that compares 64 tokens a wave step (no bucket table, no LCP table).  A range of at
 * most `stream cap` slots (sa_amd_ngram_set_stream_cap of the calling thread) is streamed once; a longer one is sampled at 64
 * slots and every run start between two differing samples is found by one binary search: at most
 * 64 + D (ceil(log2(cnt + 1)) + 1) slots probed for D distinct continuations, cnt = hi - lo - at_end.  With tokens or counts
 * asked for, the continuations are computed twice (counted, then emitted in order).
 */
typedef struct sa_amd_tok_index sa_amd_tok_index;
int32_t sa_amd_tok_index_create(const uint16_t *T, int32_t n, const uint32_t *SA, sa_amd_tok_index **out);
void sa_amd_tok_index_destroy(sa_amd_tok_index *ix);
int32_t sa_amd_tok_index_sa(const sa_amd_tok_index *ix, uint32_t *SA_out);        /* n + 1 entries */
int32_t sa_amd_tok_index_search(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi);
int32_t sa_amd_tok_index_next_tokens(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                     uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end,
                                     int64_t *list_off, uint16_t *tokens, uint32_t *counts, int64_t capacity, int64_t *total_out);
int32_t sa_amd_tok_index_infgram(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                 int32_t min_count, int32_t max_len, uint32_t *suffix_len,
                                 uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end,
                                 int64_t *list_off, uint16_t *tokens, uint32_t *counts, int64_t capacity, int64_t *total_out);

typedef struct sa_amd_tok_stats {    /* of the calling thread: the query fields of its most recent next_tokens / infgram call on a token
                                        index, the three times of its most recent token build (no other feature's statistics are touched) */
    int64_t patterns;
    int64_t range_searches;          /* infgram: the probes of the bisection, all prompts; next_tokens: one per pattern */
    int64_t compared_tokens;         /* infgram: text tokens the range searches compared; -1 after next_tokens */
    int64_t stream_slots;            /* slots probed by the streaming route: the sum of cnt over its queries, exactly */
    int64_t search_slots;            /* slots probed by the boundary-search route */
    int64_t stream_queries;          /* queries by route: 0 < cnt <= stream_cap */
    int64_t search_queries;          /*                   cnt > stream_cap */
    int64_t empty_queries;           /*                   cnt == 0: nothing is probed */
    int64_t entries;                 /* entries of the whole listing (= *total_out) */
    int32_t stream_cap;              /* the stream cap in effect */
    int32_t readbacks;               /* blocking device -> host read-backs of counters: 1 */
    int32_t backoff;                 /* 1 after infgram, 0 after next_tokens */
    int32_t passes;                  /* runs of the continuation kernel: 1 (counted only), else 2 */
    double image_ms;                 /* the most recent token build (sa_amd_saca_u16, or sa_amd_tok_index_create with SA == NULL), host
                                        time around a drained stream: the byte image, */
    double build_ms;                 /*   the byte builder on the image, */
    double compact_ms;               /*   counts, scan and scatter of the compaction */
} sa_amd_tok_stats;
void sa_amd_last_tok_stats(sa_amd_tok_stats *out);

/*
 * Scoring a token text under the infinity-gram model on the token index (an extension): for every
 * position of a query the back-off of sa_amd_tok_index_infgram and the count of the token that is really there, on the device.
 * The contract is that of sa_amd_index_infgram_score (above) with "byte" replaced by "token": T has n tokens, SA has n + 1
 * slots of the token array; "range of a string" is the [lo, hi) that sa_amd_tok_index_search reports; at_end and next[t] are
 * those of sa_amd_tok_index_next_tokens; m, q_off, S and max_len (1 .. SA_AMD_SCORE_MAX_CONTEXT) are in tokens.
 *   Q has m tokens (2 m bytes, 2-byte aligned).  q_off has ndocs + 1 entries, q_off[0] = 0, non-decreasing, q_off[ndocs] = m:
 *   document d is Q[q_off[d] .. q_off[d + 1]), empty documents are allowed.  q_off == NULL means one document [0, m) (ndocs is
 *   ignored).
 * For position j of the document that starts at `start`:
 *   cap_j  = min(j - start, max_len): a context never crosses a document start.
 *   S[j]   = the largest s in 0 .. cap_j such that Q[j - s .. j) has hi - lo >= min_count.  s = 0 always qualifies, with the
 *            range [0, n + 1) and at_end = 1.
 *   S[j], LO[j], HI[j], AT_END[j] = what sa_amd_tok_index_infgram returns as suffix_len, range and at_end for the prompt
 *            Q[start .. j) with the same min_count and max_len.
 *   NLO[j] = LO + AT_END + sum(next[t'] for t' < Q[j]),  NHI[j] = NLO + next[Q[j]].
 *   Where NHI > NLO, [NLO, NHI) is the range of Q[j - s .. j]; where the continuation does not occur, NHI == NLO is its
 *   insertion point inside the context's range.
 * The model's probability of Q[j] is (NHI - NLO) / (HI - LO - AT_END); the denominator is 0 when the context occurs only as
 * the text's last tokens.
 *   T = {256, 1, 256, 1, 2}, SA = {5, 3, 1, 4, 2, 0}, Q = {7, 256, 1, 256}, one document, min_count = 1, max_len = 4:
 *     j  token  S  [LO, HI)  AT_END  [NLO, NHI)
 *     0  7      0  [0, 6)    1       [4, 4)
 *     1  256    0  [0, 6)    1       [4, 6)
 *     2  1      1  [4, 6)    0       [4, 6)
 *     3  256    2  [4, 6)    0       [5, 6)
 *   With min_count = 3, positions 2 and 3 have S = 0: {256} occurs twice.
 * The same gallop and bisection: at most 2 ceil(log2(S[j] + 2)) + 2 range searches for position j, whatever the group cap
 * (sa_amd_score_set_group_cap of the calling thread, here counted in tokens).  A range search is a plain binary search: the
 * token index has no bucket table and no LCP table.
 * EVERY output pointer may be NULL.  m == 0 succeeds.  Errors, each with nothing written: a NULL index, m < 0, a Q that is not
 * 2-byte aligned, min_count < 1, max_len outside 1 .. SA_AMD_SCORE_MAX_CONTEXT, with q_off: ndocs < 0 or offsets that break the
 * rules above: SA_AMD_EINVAL.  If the resident array is not the suffix array of the text the answers are unspecified, but every
 * slot read lies in [0, n + 1), every SA entry is checked against n in 64 bits before T is read through it, Q is read inside
 * [0, m) only and nothing is written outside the outputs.  The answers are the same for every group cap.
 * Host pointers only: there is no device form of a token entry point.
 */
int32_t sa_amd_tok_index_infgram_score(const sa_amd_tok_index *ix, const uint16_t *Q, int64_t m, const int64_t *q_off, int64_t ndocs,
                                       int32_t min_count, int32_t max_len, uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END,
                                       uint32_t *NLO, uint32_t *NHI);

typedef struct sa_amd_tok_score_stats {  /* of the calling thread's most recent sa_amd_tok_index_infgram_score call: the fields of
                                            sa_amd_score_stats (no other feature's statistics are touched, and no other call touches these) */
    int64_t positions;               /* m */
    int64_t documents;               /* ndocs; 1 where q_off is NULL */
    int64_t group_searches;          /* range searches of the group path (8 lanes a position, the context in LDS) */
    int64_t long_searches;           /* range searches of the long path (one wave a position) */
    int64_t next_lookups;            /* slots probed by the two lower bounds on the token behind the context, all positions */
    int64_t compared_tokens;         /* text tokens the range searches compared, chunks charged whole (16 on the group path, up to 64 on the long path) */
    int64_t long_positions;          /* positions finished by the long path */
    int64_t zero_positions;          /* positions with NHI == NLO */
    int32_t group_cap;               /* the cap in effect, in tokens: min(group cap, max_len, 4096) */
    int32_t readbacks;               /* blocking device -> host read-backs of counters: 1, or 2 with long positions */
} sa_amd_tok_score_stats;
void sa_amd_last_tok_score_stats(sa_amd_tok_score_stats *out);

/* ---- per-kernel timing (HIP events on the launch stream), per calling thread ----
 * begin() zeroes and enables the counters for builds issued by this thread; end() disables them and
 * copies up to `capacity` classes out (ms = summed event time, launches, units = elements or bytes
 * processed); returns the number of kernel classes.  Used by bench.py for the roofline line. */
void sa_amd_profile_begin(void);
/* the same for a subset of the kernel classes only (bit i = class i of sa_amd_profile_kernel_name): bench.py times just
 * the dominant kernel inside its timed region -- ~300 event records per build are ~0.7 ms of host time -- and takes the
 * full per-kernel table from one extra build outside it */
void sa_amd_profile_begin_classes(uint64_t class_mask);
int32_t sa_amd_profile_end(double *ms, int64_t *launches, int64_t *units, int32_t capacity);
const char *sa_amd_profile_kernel_name(int32_t index);

#ifdef __cplusplus
}
#endif

/* Texts of 32-bit token ids below 2^24 -- sa_amd_saca_u32, sa_amd_tok32_index_* (an extension): the
 * 16-bit token forms above for tokeniser ids held in uint32_t.  Part of this interface, declared and documented in a file of
 * its own. */
#include "suffix_array_amd_tok32.h"
/* Boolean document queries -- sa_amd_index_doc_match, sa_amd_index_doc_match_list (an extension): AND, OR
 * and NOT over patterns on the collection of sa_amd_index_set_documents.  Declared and documented in a file of its own. */
#include "suffix_array_amd_docmatch.h"

#endif /* SUFFIX_ARRAY_AMD_H */
