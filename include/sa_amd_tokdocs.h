/* sa_amd_tokdocs.h -- the C ABI for document collections over the token indexes.  This file includes suffix_array_amd.h; that
 * header does not include this one: a caller who wants these calls includes this file and has everything. */
#ifndef SA_AMD_TOKDOCS_H
#define SA_AMD_TOKDOCS_H
#include "suffix_array_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Document collections over a token index (an extension): which document a token position lies in, in how
 * many documents a token n-gram occurs and in which ones, and Boolean queries over such n-grams -- what sa_amd_index_set_documents,
 * _doc_of, _doc_search, _doc_list (suffix_array_amd.h) and _doc_match, _doc_match_list (suffix_array_amd_docmatch.h) are to the
 * byte index, on sa_amd_tok_index (16-bit tokens) and sa_amd_tok32_index (ids below 2^24 in uint32_t).  The definitions, limits
 * and errors are those two headers' with "byte" read as "token": every position, offset and length counts tokens; the same
 * kernels answer, on the same tables.
 *   A collection is doc_off[0 .. ndocs], uint32: ndocs >= 1, doc_off[0] = 0, doc_off[ndocs] = n, non-decreasing; empty documents
 *     are legal anywhere.  Document d is the token range [doc_off[d], doc_off[d + 1]).
 *   doc(p) is the d with doc_off[d] <= p < doc_off[d + 1]; for p >= n it is SA_AMD_DOC_NONE (0xffffffff).
 *   D(p) is the set of documents in which an occurrence of the pattern p STARTS.  occ is by definition hi - lo of
 *     sa_amd_tok_index_search for the same pattern (the empty pattern: n + 1), df = |D(p)|; _doc_list lists D(p) in the order of
 *     the slot of each document's first occurrence in the range; _doc_match_list lists R(q) in ascending document id.
 *   T = "abracadabra" with a = 0x00ff, b = 0x0100, c = 0x01ff, d = 0x0200, r = 0xff00 (the tokens compare as the letters do; the
 *     little-endian bytes of these ids would not), doc_off = {0, 4, 4, 7, 11} (documents "abra", "", "cad", "abra"):
 *     "a" has occ 5, df 3 and the listing {3, 0, 2}; "bra" has occ 2, df 2, listing {3, 0}; "" has df 3.
 *     query                   listing     df
 *     a AND bra               {0, 3}      2
 *     a AND NOT bra           {2}         1
 *     NOT a                   {1}         1
 *     (c OR bra)              {0, 2, 3}   3
 *     ac                      {0}         1
 *     a AND c AND bra         {}          0
 *     no clauses              {0, 1, 2, 3} 4
 * _set_documents takes the caller's offsets.  _set_documents_by_separator defines the collection from the resident text: every
 *   occurrence of `separator` ends a document and belongs to it.  With p_0 < ... < p_(k-1) the positions of the separator:
 *   doc_off[0] = 0, doc_off[j + 1] = p_j + 1, and a last document runs to n when n == 0 or T[n - 1] != separator, so
 *   ndocs = k + (n == 0 || T[n - 1] != separator).  No separator at all gives one document; consecutive separators give
 *   one-token documents, never empty ones; n == 0 gives {0, 0}.  The text is read twice on the device (2 sizeof(token) n bytes),
 *   4 ndocs bytes are written, and two words come back in the whole call: k, and the error word of the build's sort.
 *   *ndocs_out (may be NULL) receives ndocs.  _doc_offsets returns the collection in effect: min(capacity, ndocs + 1) entries
 *   are written to doc_off_out (may be NULL when capacity is 0) and *ndocs_out always.
 * Calling either _set_documents form again replaces the collection; on any failure the previous collection stays.  Not to be
 * called while another thread queries the index; queries may run concurrently (the threading rule of sa_amd_index_set_documents).
 * Errors, each with nothing written: SA_AMD_EINVAL for everything the byte forms reject and for any call before a collection
 *   was set; SA_AMD_ERANGE for a pattern id that is no token (2^24 or more on the 32-bit index) and for a separator above 0xffff
 *   on the 16-bit index or of 2^24 or more on the 32-bit index -- both found before the device is touched.  A refused allocation
 *   is SA_AMD_ENOMEM with nothing written and the previous collection kept.  Outputs are written only after the last step that
 *   can fail.
 * sa_amd_docs_set_chunk and sa_amd_doc_match_set_budget apply, and the calls fill the calling thread's sa_amd_last_docs_stats /
 * sa_amd_last_doc_match_stats records: they run the byte index's routes.  Host pointers only: there is no device form.
 */
int32_t sa_amd_tok_index_set_documents(sa_amd_tok_index *ix, const uint32_t *doc_off, int64_t ndocs);
int32_t sa_amd_tok_index_set_documents_by_separator(sa_amd_tok_index *ix, uint32_t separator, int64_t *ndocs_out);
int32_t sa_amd_tok_index_doc_offsets(const sa_amd_tok_index *ix, uint32_t *doc_off_out, int64_t capacity, int64_t *ndocs_out);
/* pos (count entries, any values) goes up, doc(pos[i]) comes back */
int32_t sa_amd_tok_index_doc_of(const sa_amd_tok_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out);
/* patterns as for sa_amd_tok_index_search; occ and df: count entries each, either may be NULL */
int32_t sa_amd_tok_index_doc_search(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                    uint32_t *occ, uint32_t *df);
/* the listing of pattern q is docs[list_off[q] .. list_off[q + 1]) (list_off: count + 1 entries).  More entries than fit is no
 * error: the first `capacity` are written, *total_out (= list_off[count]) and list_off describe all of them. */
int32_t sa_amd_tok_index_doc_list(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t count,
                                  int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out);
/* clauses and queries as for sa_amd_index_doc_match; df: nqueries entries, clause_df: nclauses entries; either may be NULL */
int32_t sa_amd_tok_index_doc_match(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t npat,
                                   const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                                   const int32_t *query_off, int32_t nqueries, uint32_t *df, uint32_t *clause_df);
int32_t sa_amd_tok_index_doc_match_list(const sa_amd_tok_index *ix, const uint16_t *pat_data, const int64_t *pat_off, int32_t npat,
                                        const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                                        const int32_t *query_off, int32_t nqueries, int64_t *list_off, uint32_t *docs,
                                        int64_t capacity, int64_t *total_out);

/* the same calls on the 32-bit token index: uint32_t patterns, every id below SA_AMD_TOKEN_LIMIT_U32 */
int32_t sa_amd_tok32_index_set_documents(sa_amd_tok32_index *ix, const uint32_t *doc_off, int64_t ndocs);
int32_t sa_amd_tok32_index_set_documents_by_separator(sa_amd_tok32_index *ix, uint32_t separator, int64_t *ndocs_out);
int32_t sa_amd_tok32_index_doc_offsets(const sa_amd_tok32_index *ix, uint32_t *doc_off_out, int64_t capacity, int64_t *ndocs_out);
int32_t sa_amd_tok32_index_doc_of(const sa_amd_tok32_index *ix, const uint32_t *pos, int64_t count, uint32_t *doc_out);
int32_t sa_amd_tok32_index_doc_search(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                      uint32_t *occ, uint32_t *df);
int32_t sa_amd_tok32_index_doc_list(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t count,
                                    int64_t *list_off, uint32_t *docs, int64_t capacity, int64_t *total_out);
int32_t sa_amd_tok32_index_doc_match(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t npat,
                                     const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                                     const int32_t *query_off, int32_t nqueries, uint32_t *df, uint32_t *clause_df);
int32_t sa_amd_tok32_index_doc_match_list(const sa_amd_tok32_index *ix, const uint32_t *pat_data, const int64_t *pat_off, int32_t npat,
                                          const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                                          const int32_t *query_off, int32_t nqueries, int64_t *list_off, uint32_t *docs,
                                          int64_t capacity, int64_t *total_out);

#ifdef __cplusplus
}
#endif
#endif /* SA_AMD_TOKDOCS_H */
