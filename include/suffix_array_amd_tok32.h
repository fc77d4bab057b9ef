/* suffix_array_amd_tok32.h -- the C ABI for texts of 32-bit token ids below 2^24.  suffix_array_amd.h includes this file: a
 * caller includes that one and has both. */
#ifndef SUFFIX_ARRAY_AMD_TOK32_H
#define SUFFIX_ARRAY_AMD_TOK32_H
#include "suffix_array_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Texts of 32-bit token ids below 2^24 (an extension): what suffix_array_amd.h gives for 16-bit tokens
 * ("Texts over a 16-bit token alphabet", "Scoring a token text under the infinity-gram model"), for the vocabularies of 100 k to 262 k entries whose corpora are stored as uint32 arrays.  Everything said there holds with
 * "16-bit token" replaced by "token id in a uint32_t, value < SA_AMD_TOKEN_LIMIT_U32": T has n tokens compared as unsigned
 * values, a suffix that is a proper prefix of another sorts first, SA has n + 1 entries in TOKEN positions and SA[0] = n;
 * lengths, pat_off, suffix_len, max_len, m and q_off count tokens; a listing has at most min(2^24, hi - lo) entries in
 * ascending token value and its token output is uint32_t; Q is 4-byte aligned.  The 16-bit forms on the ids truncated to 16
 * bits are NOT a substitute (the example below), and neither are the raw bytes.
 * Construction: the big-endian image of T at THREE bytes a token (3 n bytes: a quarter less than the four stored) goes through
 * the byte builder, and an order-preserving compaction keeps the entries of its array that are divisible by 3, divided by 3.
 * Peak device memory of sa_amd_saca_u32: 4 n (T) + 3 n + 16 (image) + 4 (3 n + 1) + sa_amd_workspace_bytes(3 n), one pooled
 * block; a block that does not fit is SA_AMD_ENOMEM (no reduced-memory route).  The index keeps T (4 n bytes) and the array.
 * n == 0 gives SA = {0}.  n < 0, n > sa_amd_max_tokens_u32(), a NULL SA (saca), a NULL T with n > 0: SA_AMD_EINVAL.
 * A token of T that is not below 2^24: SA_AMD_ERANGE.  The text is checked on the device, by sa_amd_saca_u32 and by
 * sa_amd_tok32_index_create with and without a supplied array, before the byte builder starts: nothing is built, SA / *out are
 * not written (*out is NULL).  A supplied array is checked as the 16-bit form checks it: an entry above n is SA_AMD_ERANGE,
 * SA[0] != n is SA_AMD_EINVAL.
 * A pattern, prompt or query token that is not below 2^24: SA_AMD_ERANGE, from a scan on the host before anything is uploaded,
 * with nothing written; it is answered after the SA_AMD_EINVAL checks of the 16-bit forms, which are the same here.
 *   T = {65537, 1, 65536, 1, 2}, SA = {5, 3, 1, 4, 2, 0}.  Truncated to 16 bits the ids are {1, 1, 0, 1, 2}, whose array is
 *   {5, 2, 1, 0, 3, 4}: another order.
 *     context      range     at_end  listing
 *     {65536, 1}   [4, 5)    0       {2:1}
 *     {1}          [1, 3)    0       {2:1, 65536:1}
 *     {2}          [3, 4)    1       empty
 *     {}           [0, 6)    1       {1:2, 2:1, 65536:1, 65537:1}
 *     {9}          empty     0       empty
 *     prompt         min_count max_len  s   range
 *     {7, 65536, 1}  1         none     2   [4, 5)
 *     {7, 65536, 1}  2         none     1   [1, 3)
 *     {7, 65536, 1}  3         none     0   [0, 6)
 *   Q = {7, 65536, 1, 2}, one document, min_count = 1, max_len = 4 (sa_amd_tok32_index_infgram_score):
 *     j  token  S  [LO, HI)  AT_END  [NLO, NHI)
 *     0  7      0  [0, 6)    1       [4, 4)
 *     1  65536  0  [0, 6)    1       [4, 5)
 *     2  1      1  [4, 5)    0       [4, 5)
 *     3  2      2  [4, 5)    0       [4, 5)
 * Statistics: sa_amd_last_tok_stats and sa_amd_last_tok_score_stats (suffix_array_amd.h) describe the calling thread's latest token call of
 * either width.  sa_amd_ngram_set_stream_cap and sa_amd_score_set_group_cap apply as they do to the 16-bit forms.
 * Host pointers only: there is no device form of a token entry point.
 */
#define SA_AMD_TOKEN_LIMIT_U32 (1 << 24)
int32_t sa_amd_max_tokens_u32(void);                                              /* 715827882 = (2^31 - 1) / 3 */
int32_t sa_amd_saca_u32(const uint32_t *T, uint32_t *SA, int32_t n);              /* host pointers */
typedef struct sa_amd_tok32_index sa_amd_tok32_index;
int32_t sa_amd_tok32_index_create(const uint32_t *T, int32_t n, const uint32_t *SA, sa_amd_tok32_index **out);
void sa_amd_tok32_index_destroy(sa_amd_tok32_index *ix);
int32_t sa_amd_tok32_index_sa(const sa_amd_tok32_index *ix, uint32_t *SA_out);    /* n + 1 entries */
int32_t sa_amd_tok32_index_search(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                  uint8_t *contains, uint32_t *range_lo, uint32_t *range_hi);
int32_t sa_amd_tok32_index_next_tokens(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                       uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end,
                                       int64_t *list_off, uint32_t *tokens, uint32_t *counts, int64_t capacity, int64_t *total_out);
int32_t sa_amd_tok32_index_infgram(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                   int32_t min_count, int32_t max_len, uint32_t *suffix_len,
                                   uint32_t *range_lo, uint32_t *range_hi, uint8_t *at_end,
                                   int64_t *list_off, uint32_t *tokens, uint32_t *counts, int64_t capacity, int64_t *total_out);
int32_t sa_amd_tok32_index_infgram_score(const sa_amd_tok32_index *ix, const uint32_t *Q, int64_t m, const int64_t *q_off, int64_t ndocs,
                                         int32_t min_count, int32_t max_len, uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END,
                                         uint32_t *NLO, uint32_t *NHI);

#ifdef __cplusplus
}
#endif
#endif /* SUFFIX_ARRAY_AMD_TOK32_H */
