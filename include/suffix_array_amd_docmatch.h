/* suffix_array_amd_docmatch.h -- the C ABI for Boolean document queries over the device index.  suffix_array_amd.h includes this
 * file: a caller includes that one and has both. */
#ifndef SUFFIX_ARRAY_AMD_DOCMATCH_H
#define SUFFIX_ARRAY_AMD_DOCMATCH_H
#include "suffix_array_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Boolean document queries (an extension): which documents of the index's collection hold this pattern
 * AND that one, this one OR that one, this one but NOT that one -- answered on the device from the tables that
 * sa_amd_index_set_documents left there, without a listing crossing to the host to be intersected.
 *   The collection is doc_off[0 .. ndocs], as sa_amd_index_set_documents took it.
 *   For a pattern p, D(p) is the set of documents in which an occurrence of p STARTS: exactly the set sa_amd_index_doc_list
 *     lists.  The empty suffix belongs to no document; the empty pattern gives the non-empty documents.
 *   A CLAUSE c is a list of patterns and a flag byte; bit 0 of the flag byte means "negated".
 *     U(c) = the union of D(p) over its patterns; a clause with no patterns has U = {}.
 *     S(c) = U(c) when not negated, {0 .. ndocs - 1} \ U(c) when negated: empty documents are in every negated clause's set.
 *   A QUERY q is a list of clauses.  R(q) = the intersection of S(c) over its clauses; a query with no clauses has
 *     R = {0 .. ndocs - 1}, empty documents included.
 *   df[q] = |R(q)|, clause_df[c] = |S(c)|, and the listing of q is R(q) in ASCENDING DOCUMENT ID.  That is not the slot order of
 *     sa_amd_index_doc_list: the result comes from a bitmap, and ascending is the order that costs no sort.
 *   T = "abracadabra", doc_off = {0, 4, 4, 7, 11} (documents "abra", "", "cad", "abra"):
 *     query                   listing     df
 *     a AND bra               {0, 3}      2
 *     a AND NOT bra           {2}         1
 *     NOT a                   {1}         1
 *     (c OR bra)              {0, 2, 3}   3
 *     ac                      {0}         1
 *     a AND c AND bra         {}          0
 *     no clauses              {0, 1, 2, 3} 4
 *     "ac" matches across the boundary at byte 3 and starts in document 0.
 * Arguments: the patterns as for sa_amd_index_search (pat_data, pat_off, npat).  Clause c holds the patterns
 *   [clause_off[c], clause_off[c + 1]): clause_off has nclauses + 1 entries, starts at 0, never decreases and ends at npat.
 *   Query q holds the clauses [query_off[q], query_off[q + 1]): query_off has nqueries + 1 entries, starts at 0, never decreases
 *   and ends at nclauses.  So every pattern belongs to one clause and every clause to one query; a pattern or clause that is to
 *   serve twice is passed twice.  clause_flags has nclauses bytes, or is NULL: no clause is negated.  Bits other than bit 0 must
 *   be 0.
 * Errors, each with nothing written and no device touched, are SA_AMD_EINVAL: a NULL index, a call before
 *   sa_amd_index_set_documents, negative counts or capacity, pat_off as sa_amd_index_search rejects it, clause_off or query_off
 *   that break the rules above (NULL included), unknown flag bits, a NULL list_off or total_out, NULL docs with capacity > 0.
 *   A refused allocation is SA_AMD_ENOMEM with nothing written.  With nqueries == 0 the call returns at once, with
 *   list_off[0] = 0 and *total_out = 0.  Outputs are written only after the last step that can fail.  If the resident array is
 *   no suffix array the answers are unspecified; nothing is read outside the tables and nothing is written outside the outputs.
 * How: the ranges and units of all patterns as sa_amd_index_doc_search computes them (sa_amd_docs_set_chunk applies), with its
 *   one blocking read-back.  One bitmap of W = ceil(ndocs / 32) words per clause: the slots that are the first of their document
 *   in a range -- one compare of the per-slot word -- set their document's bit, so a call issues sum |D(p)| atomics and streams
 *   4 bytes per occurrence.  A pass over (query, 256-word tile) ANDs the clauses' words, complemented where negated, and counts;
 *   a listing adds one 64-bit scan over the tiles' counts and a pass that writes the set bits.  Consecutive whole queries share a
 *   SLAB while their clauses' bitmaps (4 W bytes each) fit the budget; slabs run one after another without a read-back.
 * Host pointers only: there is no device form.  The threading rule of sa_amd_index_set_documents applies.
 */
/* df: nqueries entries, clause_df: nclauses entries; either may be NULL */
int32_t sa_amd_index_doc_match(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t npat,
                               const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                               const int32_t *query_off, int32_t nqueries, uint32_t *df, uint32_t *clause_df);
/* the listing of query q is docs[list_off[q] .. list_off[q + 1]) (list_off: nqueries + 1 entries).  More entries than fit is no
 * error: the first `capacity` entries are written and *total_out says how many there are, as for sa_amd_index_doc_list */
int32_t sa_amd_index_doc_match_list(const sa_amd_index *ix, const uint8_t *pat_data, const int64_t *pat_off, int32_t npat,
                                    const int32_t *clause_off, const uint8_t *clause_flags, int32_t nclauses,
                                    const int32_t *query_off, int32_t nqueries, int64_t *list_off, uint32_t *docs, int64_t capacity,
                                    int64_t *total_out);

typedef struct sa_amd_doc_match_stats { /* of the calling thread's most recent doc_match / doc_match_list call; every field is a function of the inputs */
    int64_t patterns;
    int64_t clauses;
    int64_t queries;
    int64_t occ_sum;                 /* occurrences of all patterns: the per-slot words streamed by a counting call */
    int64_t units;                   /* sum over the patterns of ceil(occ / chunk) */
    int64_t marks;                   /* sum over the patterns of |D(p)|: the atomics that set a bit */
    int64_t bitmap_words;            /* W = ceil(ndocs / 32) */
    int64_t slabs;                   /* 0 when nqueries == 0 */
    int64_t df_sum;                  /* sum of df over the queries (the listing's total after doc_match_list) */
    int64_t budget;                  /* bytes of bitmaps a slab may hold (sa_amd_doc_match_set_budget) */
    int32_t chunk;                   /* slots per unit in effect (sa_amd_docs_set_chunk) */
    int32_t readbacks;               /* blocking read-backs: 1, the number of units (0 when there is no pattern); a listing's
                                      * list_off comes down behind the last kernel, as sa_amd_index_doc_list's does */
    int32_t listed;                  /* 1 after doc_match_list, 0 after doc_match */
    int32_t reserved;
} sa_amd_doc_match_stats;
/* sa_amd_last_docs_stats and the other features' statistics are not touched by these calls, nor these by theirs */
void sa_amd_last_doc_match_stats(sa_amd_doc_match_stats *out);
/* route switch of the calling thread's later doc_match / doc_match_list calls (never changes a result): the bytes of clause
 * bitmaps one slab may hold, clamped to 4 KiB .. 2^40; a negative value restores the default of 256 MiB.  Returns the
 * previous value. */
int64_t sa_amd_doc_match_set_budget(int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SUFFIX_ARRAY_AMD_DOCMATCH_H */
