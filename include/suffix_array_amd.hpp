// suffix_array_amd.hpp -- C++ host-side mirror of the reference's construction interface, over
// the C ABI of suffix_array_amd.h.  Same names, argument meaning and error behaviour as the
// Rust crate for the path in scope:
//   saca(), MAX_LENGTH                      reference src/saca.rs:6-15
//   SuffixArray::new_/set/len/is_empty/into_parts/from_parts/unchecked_from_parts
//                                           reference src/sa.rs:23-70, check_integrity src/sa.rs:72-84
//   SuffixArray::enable_buckets / buckets   reference src/sa.rs:89-119 (the table, built on the GPU from the text alone)
//   SuffixArray::lcp_array                  EXTENSION: the LCP array (the reference's README TODO "enhanced suffix array")
//   SuffixArray::bwt, bwt(), unbwt()        EXTENSION: the Burrows-Wheeler transform and its inverse (divbwt /
//                                           inverse_bw_transform of the C engine the reference binds)
//   SuffixArray::repeat_lengths / repeat_spans, repeat_lengths(), repeat_spans()
//                                           EXTENSION: the longest-repeat array and the byte ranges that are copies
//   SuffixArray::repeated_substrings, repeated_substrings()
//                                           EXTENSION: the substrings that occur at least twice, as suffix-tree nodes: all of
//                                           them or the k most frequent, longest or most covering
//   DocumentIndex                           EXTENSION: a device-resident index over a collection of documents: which document a
//                                           position lies in, in how many documents a pattern occurs and in which ones,
//                                           (term_frequencies, top_k) how often in each and the k documents with the most
//                                           occurrences, (repeat_spans) the duplicate byte ranges that respect the
//                                           document boundaries, and (repeated_substrings) the repeated substrings with the
//                                           number of documents each occurs in
// Rust panics (assert!, engine failure) are std::logic_error / std::runtime_error here.
#pragma once
#include "suffix_array_amd.h"
#include "sa_amd_tokdocs.h"

#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace suffix_array {

constexpr std::size_t MAX_LENGTH = SA_AMD_MAX_LENGTH;            // src/saca.rs:6

// pub fn saca(s: &[u8], sa: &mut [u32])                          // src/saca.rs:9-15
inline void saca(const std::uint8_t *s, std::size_t n, std::uint32_t *sa, std::size_t sa_len)
{
    if (n > MAX_LENGTH) throw std::logic_error("assertion failed: s.len() <= MAX_LENGTH");      // :10
    if (n + 1 != sa_len) throw std::logic_error("assertion failed: s.len() + 1 == sa.len()");   // :11
    const std::int32_t rc = sa_amd_saca_u8(s, sa, static_cast<std::int32_t>(n));                 // :13-14
    if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
}

// EXTENSION: the Burrows-Wheeler transform of s (layout in suffix_array_amd.h): n bytes and the primary index.  sa == nullptr:
// the suffix array is built on the device and never downloaded (sa_amd_bwt)
inline std::pair<std::vector<std::uint8_t>, std::int32_t> bwt(const std::uint8_t *s, std::size_t n, const std::uint32_t *sa = nullptr)
{
    if (n > MAX_LENGTH) throw std::logic_error("assertion failed: s.len() <= MAX_LENGTH");
    std::vector<std::uint8_t> b(n);
    std::int32_t primary = 0;
    const std::int32_t rc = sa_amd_bwt(s, static_cast<std::int32_t>(n), sa, b.data(), &primary);
    if (rc == SA_AMD_ERANGE) throw std::out_of_range("suffix offset out of range");
    if (rc == SA_AMD_EINVAL) throw std::invalid_argument("not a suffix array of this layout");
    if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    return { std::move(b), primary };
}

// EXTENSION: the longest-repeat array of s (suffix_array_amd.h): n entries in text order.  sa == nullptr: the suffix array is
// built on the device and never downloaded (sa_amd_repeat_lengths)
inline std::vector<std::uint32_t> repeat_lengths(const std::uint8_t *s, std::size_t n, const std::uint32_t *sa = nullptr)
{
    if (n > MAX_LENGTH) throw std::logic_error("assertion failed: s.len() <= MAX_LENGTH");
    std::vector<std::uint32_t> lr(n);
    const std::int32_t rc = sa_amd_repeat_lengths(s, static_cast<std::int32_t>(n), sa, lr.data());
    if (rc == SA_AMD_ERANGE) throw std::out_of_range("suffix offset out of range");
    if (rc == SA_AMD_EINVAL) throw std::invalid_argument("not a suffix array of this layout");
    if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    return lr;
}

// EXTENSION: the byte ranges of s that are copies, as [start, end) pairs, ascending, disjoint and not adjacent: every occurrence of
// a substring of at least min_len bytes that occurs twice, or (keep_first) every window of min_len bytes that equals an earlier
// one (sa_amd_repeat_spans).  Only the spans come back from the device.
inline std::vector<std::pair<std::uint32_t, std::uint32_t>> repeat_spans(const std::uint8_t *s, std::size_t n, std::int32_t min_len,
                                                                         bool keep_first = false, const std::uint32_t *sa = nullptr)
{
    if (n > MAX_LENGTH) throw std::logic_error("assertion failed: s.len() <= MAX_LENGTH");
    if (min_len < 1) throw std::invalid_argument("min_len must be at least 1");
    const std::int64_t cap = sa_amd_repeat_spans_bound(static_cast<std::int32_t>(n), min_len);
    std::vector<std::uint32_t> flat(static_cast<std::size_t>(cap) * 2);
    std::int64_t count = 0;
    const std::int32_t rc = sa_amd_repeat_spans(s, static_cast<std::int32_t>(n), sa, min_len,
                                                keep_first ? SA_AMD_REPEATS_KEEP_FIRST : SA_AMD_REPEATS_ALL, flat.data(), cap, &count);
    if (rc == SA_AMD_ERANGE) throw std::out_of_range("suffix offset out of range");
    if (rc == SA_AMD_EINVAL) throw std::invalid_argument("not a suffix array of this layout");
    if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    std::vector<std::pair<std::uint32_t, std::uint32_t>> out(static_cast<std::size_t>(count < cap ? count : cap));
    for (std::size_t i = 0; i < out.size(); ++i) out[i] = { flat[2 * i], flat[2 * i + 1] };
    return out;
}

// EXTENSION: the substrings of s that occur at least twice (suffix_array_amd.h, "Repeated substrings"): one row per internal node
// of the suffix tree -- the substring s[pos .. pos + depth) occurs exactly `count` times, at sa[lo .. lo + count), and so does
// every prefix of it longer than `parent`.  order SA_AMD_SUBSTR_ALL: every selected node in suffix-array order; the ranked
// orders: the best k by count, length or count * length (sa_amd_substrings).  Only the rows come back from the device.
struct RepeatedSubstring {
    std::uint32_t lo, count, depth, parent;
    std::uint32_t pos;                                            // sa[lo]: where the substring can be read
    bool operator==(const RepeatedSubstring &o) const
    {
        return lo == o.lo && count == o.count && depth == o.depth && parent == o.parent && pos == o.pos;
    }
    bool operator!=(const RepeatedSubstring &o) const { return !(*this == o); }
};
inline std::vector<RepeatedSubstring> repeated_substrings(const std::uint8_t *s, std::size_t n, std::int32_t min_len = 1, std::int32_t max_len = 0,
                                                          std::int32_t min_count = 2, std::int32_t order = SA_AMD_SUBSTR_ALL, std::int64_t k = 0,
                                                          const std::uint32_t *sa = nullptr)
{
    if (n > MAX_LENGTH) throw std::logic_error("assertion failed: s.len() <= MAX_LENGTH");
    const sa_amd_substr_query q = { min_len, max_len, min_count, order, k };
    std::int64_t cap = sa_amd_substrings_bound(static_cast<std::int32_t>(n));
    if (order != SA_AMD_SUBSTR_ALL && k >= 1 && k < cap) cap = k;
    std::vector<std::uint32_t> flat(static_cast<std::size_t>(cap) * 4), pos(static_cast<std::size_t>(cap));
    std::int64_t total = 0;
    const std::int32_t rc = sa_amd_substrings(s, static_cast<std::int32_t>(n), sa, &q, flat.data(), pos.data(), cap, &total);
    if (rc == SA_AMD_ERANGE) throw std::out_of_range("suffix offset out of range");
    if (rc == SA_AMD_EINVAL) throw std::invalid_argument("not a query of this feature / not a suffix array of this layout");
    if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    std::vector<RepeatedSubstring> out(static_cast<std::size_t>(total < cap ? total : cap));
    for (std::size_t i = 0; i < out.size(); ++i) out[i] = { flat[4 * i], flat[4 * i + 1], flat[4 * i + 2], flat[4 * i + 3], pos[i] };
    return out;
}

// EXTENSION: the text whose transform is (b, primary); std::invalid_argument when the pair is not a transform (sa_amd_unbwt)
inline std::vector<std::uint8_t> unbwt(const std::uint8_t *b, std::size_t n, std::int32_t primary)
{
    if (n > MAX_LENGTH) throw std::logic_error("assertion failed: b.len() <= MAX_LENGTH");
    std::vector<std::uint8_t> t(n);
    const std::int32_t rc = sa_amd_unbwt(b, static_cast<std::int32_t>(n), primary, t.data());
    if (rc == SA_AMD_EINVAL) throw std::invalid_argument("not a Burrows-Wheeler transform");
    if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    return t;
}

class SuffixArray {
public:
    // SuffixArray::new                                            // src/sa.rs:23-27
    static SuffixArray new_(const std::uint8_t *s, std::size_t n)
    {
        SuffixArray r(s, n, std::vector<std::uint32_t>(n + 1, 0));
        saca(s, n, r.sa_.data(), r.sa_.size());
        return r;
    }
    // SuffixArray::set: re-runs construction into the resized buffer; like the reference it does
    // not replace the stored text                                 // src/sa.rs:30-33
    void set(const std::uint8_t *s, std::size_t n)
    {
        sa_.resize(n + 1, 0);
        saca(s, n, sa_.data(), sa_.size());
    }
    void fit() { sa_.shrink_to_fit(); }                           // src/sa.rs:36-38
    std::size_t len() const { return n_; }                        // src/sa.rs:41-43
    bool is_empty() const { return n_ == 0; }                     // src/sa.rs:46-48
    std::pair<const std::uint8_t *, std::vector<std::uint32_t>> into_parts() &&   // src/sa.rs:51-53
    {
        return { s_, std::move(sa_) };
    }
    const std::vector<std::uint32_t> &sa() const { return sa_; }
    // from_parts: compose and check the integrity                 // src/sa.rs:57-64
    static std::optional<SuffixArray> from_parts(const std::uint8_t *s, std::size_t n, std::vector<std::uint32_t> sa)
    {
        SuffixArray r(s, n, std::move(sa));
        if (r.check_integrity()) return r;
        return std::nullopt;
    }
    static SuffixArray unchecked_from_parts(const std::uint8_t *s, std::size_t n, std::vector<std::uint32_t> sa)
    {
        return SuffixArray(s, n, std::move(sa));                  // src/sa.rs:68-70
    }
    // enable_buckets: 256 * 257 + 1 right bucket edges in the layout of src/sa.rs:94, from the bigram counts of the text
    // (src/sa.rs:96-116); a second call is a no-op like the reference's (src/sa.rs:90-92)
    void enable_buckets()
    {
        if (!bkt_.empty()) return;
        std::vector<std::uint32_t> b(SA_AMD_BUCKET_TABLE_LEN);
        const std::int32_t rc = sa_amd_bucket_table(s_, static_cast<std::int32_t>(n_), nullptr, b.data());
        if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
        bkt_ = std::move(b);
    }
    const std::vector<std::uint32_t> &buckets() const { return bkt_; }     // empty: not enabled (the reference's bkt: None)
    // EXTENSION (not in the reference): the LCP array aligned with sa(), n + 1 entries, lcp[0] = 0, lcp[i] = longest common
    // prefix of the suffixes at sa[i-1] and sa[i]; computed on the GPU (sa_amd_lcp)
    std::vector<std::uint32_t> lcp_array() const
    {
        if (n_ + 1 != sa_.size()) throw std::logic_error("assertion failed: s.len() + 1 == sa.len()");
        std::vector<std::uint32_t> l(n_ + 1);
        const std::int32_t rc = sa_amd_lcp(s_, static_cast<std::int32_t>(n_), sa_.data(), l.data());
        if (rc == SA_AMD_ERANGE) throw std::out_of_range("suffix offset out of range");
        if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
        return l;
    }
    // EXTENSION (not in the reference): the Burrows-Wheeler transform from the text and this array (sa_amd_bwt)
    std::pair<std::vector<std::uint8_t>, std::int32_t> bwt() const
    {
        if (n_ + 1 != sa_.size()) throw std::logic_error("assertion failed: s.len() + 1 == sa.len()");
        return suffix_array::bwt(s_, n_, sa_.data());
    }
    // EXTENSION (not in the reference): the longest-repeat array and the duplicate spans from the text and this array
    std::vector<std::uint32_t> repeat_lengths() const
    {
        if (n_ + 1 != sa_.size()) throw std::logic_error("assertion failed: s.len() + 1 == sa.len()");
        return suffix_array::repeat_lengths(s_, n_, sa_.data());
    }
    std::vector<std::pair<std::uint32_t, std::uint32_t>> repeat_spans(std::int32_t min_len, bool keep_first = false) const
    {
        if (n_ + 1 != sa_.size()) throw std::logic_error("assertion failed: s.len() + 1 == sa.len()");
        return suffix_array::repeat_spans(s_, n_, min_len, keep_first, sa_.data());
    }
    // EXTENSION (not in the reference): the substrings that occur at least twice, from the text and this array
    std::vector<RepeatedSubstring> repeated_substrings(std::int32_t min_len = 1, std::int32_t max_len = 0, std::int32_t min_count = 2,
                                                       std::int32_t order = SA_AMD_SUBSTR_ALL, std::int64_t k = 0) const
    {
        if (n_ + 1 != sa_.size()) throw std::logic_error("assertion failed: s.len() + 1 == sa.len()");
        return suffix_array::repeated_substrings(s_, n_, min_len, max_len, min_count, order, k, sa_.data());
    }

private:
    SuffixArray(const std::uint8_t *s, std::size_t n, std::vector<std::uint32_t> sa) : s_(s), n_(n), sa_(std::move(sa)) {}
    bool check_integrity() const                                   // src/sa.rs:72-84 (literal form)
    {
        if (n_ + 1 != sa_.size()) return false;
        for (std::size_t i = 1; i < sa_.size(); ++i) {
            const std::size_t a = sa_[i - 1], b = sa_[i];
            if (a > n_ || b > n_) throw std::out_of_range("suffix offset out of range");   // slice index panics
            const std::size_t la = n_ - a, lb = n_ - b, l = la < lb ? la : lb;
            int c = l ? std::memcmp(s_ + a, s_ + b, l) : 0;
            if (c == 0) c = (la > lb) - (la < lb);
            if (c >= 0) return false;
        }
        return true;
    }
    const std::uint8_t *s_;
    std::size_t n_;
    std::vector<std::uint32_t> sa_;
    std::vector<std::uint32_t> bkt_;
};

// A clause of DocumentIndex::match / match_list: the documents that hold ANY of the patterns, or with `negate` those that hold none
// (written once over the pattern type: byte strings here, token sequences for TokenIndex::match)
template <class Pattern>
struct BasicClause {
    std::vector<Pattern> any;
    bool negate = false;
};
using Clause = BasicClause<std::string>;

// EXTENSION (not in the reference): text + suffix array resident on the device (sa_amd_index) with a collection of documents
// over it (suffix_array_amd.h, "Document collections over the index").  offsets: ndocs + 1 non-decreasing values from 0 to n.
class DocumentIndex {
public:
    // sa == nullptr: the suffix array is built on the device and never downloaded
    DocumentIndex(const std::uint8_t *s, std::size_t n, const std::vector<std::uint32_t> &offsets, const std::uint32_t *sa = nullptr)
    {
        if (n > MAX_LENGTH) throw std::logic_error("assertion failed: s.len() <= MAX_LENGTH");
        check(sa_amd_index_create(s, static_cast<std::int32_t>(n), sa, &ix_));
        n_ = n;
        try { set_documents(offsets); } catch (...) { sa_amd_index_destroy(ix_); throw; }
    }
    DocumentIndex(const DocumentIndex &) = delete;
    DocumentIndex &operator=(const DocumentIndex &) = delete;
    ~DocumentIndex() { sa_amd_index_destroy(ix_); }

    // replaces the collection; malformed offsets throw std::invalid_argument and leave the previous one in place
    void set_documents(const std::vector<std::uint32_t> &offsets)
    {
        if (offsets.size() < 2) throw std::invalid_argument("document offsets: ndocs + 1 values from 0 to n");
        check(sa_amd_index_set_documents(ix_, offsets.data(), static_cast<std::int64_t>(offsets.size()) - 1));
        ndocs_ = offsets.size() - 1;
    }
    // the document of every position; SA_AMD_DOC_NONE for positions >= n
    std::vector<std::uint32_t> doc_of(const std::vector<std::uint32_t> &positions) const
    {
        std::vector<std::uint32_t> out(positions.size());
        check(sa_amd_index_doc_of(ix_, positions.data(), static_cast<std::int64_t>(positions.size()), out.data()));
        return out;
    }
    // per pattern (occ, df): occurrences, and the number of distinct documents an occurrence starts in
    std::vector<std::pair<std::uint32_t, std::uint32_t>> doc_search(const std::vector<std::string> &patterns) const
    {
        const Batch b(patterns);
        std::vector<std::uint32_t> occ(patterns.size()), df(patterns.size());
        check(sa_amd_index_doc_search(ix_, b.data(), b.off.data(), b.count(), occ.data(), df.data()));
        std::vector<std::pair<std::uint32_t, std::uint32_t>> out(patterns.size());
        for (std::size_t q = 0; q < out.size(); ++q) out[q] = { occ[q], df[q] };
        return out;
    }
    // per pattern the distinct documents it occurs in, ordered by the document's lexicographically smallest matching suffix
    std::vector<std::vector<std::uint32_t>> doc_list(const std::vector<std::string> &patterns) const
    {
        const Batch b(patterns);
        std::vector<std::int64_t> loff(patterns.size() + 1);
        std::vector<std::uint32_t> docs(1 << 16);
        std::int64_t total = 0;
        for (;;) {
            check(sa_amd_index_doc_list(ix_, b.data(), b.off.data(), b.count(), loff.data(), docs.data(), static_cast<std::int64_t>(docs.size()), &total));
            if (total <= static_cast<std::int64_t>(docs.size())) break;
            docs.resize(static_cast<std::size_t>(total));
        }
        std::vector<std::vector<std::uint32_t>> out(patterns.size());
        for (std::size_t q = 0; q < out.size(); ++q) out[q].assign(docs.begin() + loff[q], docs.begin() + loff[q + 1]);
        return out;
    }
    // Boolean document queries (suffix_array_amd_docmatch.h): a query is the AND of its clauses, a clause the OR of its patterns,
    // negated where `negate` is set.  -> per query the number of documents it holds in; a query without clauses holds in all.
    std::vector<std::uint32_t> match(const std::vector<std::vector<Clause>> &queries) const
    {
        const Queries q(queries);
        std::vector<std::uint32_t> df(queries.size() + 1);
        check(sa_amd_index_doc_match(ix_, q.b.data(), q.b.off.data(), q.b.count(), q.coff.data(), q.flags.data(), q.clauses(), q.qoff.data(), q.count(),
                                     df.data(), nullptr));
        df.resize(queries.size());
        return df;
    }
    // per query the documents it holds in, in ascending document id
    std::vector<std::vector<std::uint32_t>> match_list(const std::vector<std::vector<Clause>> &queries) const
    {
        const Queries q(queries);
        std::vector<std::int64_t> loff(queries.size() + 1);
        std::vector<std::uint32_t> docs(1 << 16);
        std::int64_t total = 0;
        for (;;) {
            check(sa_amd_index_doc_match_list(ix_, q.b.data(), q.b.off.data(), q.b.count(), q.coff.data(), q.flags.data(), q.clauses(), q.qoff.data(),
                                              q.count(), loff.data(), docs.data(), static_cast<std::int64_t>(docs.size()), &total));
            if (total <= static_cast<std::int64_t>(docs.size())) break;
            docs.resize(static_cast<std::size_t>(total));
        }
        std::vector<std::vector<std::uint32_t>> out(queries.size());
        for (std::size_t i = 0; i < out.size(); ++i) out[i].assign(docs.begin() + loff[i], docs.begin() + loff[i + 1]);
        return out;
    }
    // keeps the slots ordered by document (4 bytes per byte of text) that term_frequencies and top_k need; a no-op when they
    // exist.  set_documents drops them: enable again after replacing the collection.
    void enable_frequencies() { check(sa_amd_index_enable_doc_freq(ix_)); }
    // per pattern the listing of doc_list as (doc, tf) pairs: tf = the occurrences that start in the document
    std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> term_frequencies(const std::vector<std::string> &patterns) const
    {
        const Batch b(patterns);
        std::vector<std::int64_t> loff(patterns.size() + 1);
        std::vector<std::uint32_t> docs(1 << 16), tf(1 << 16);
        std::int64_t total = 0;
        for (;;) {
            check(sa_amd_index_doc_tf(ix_, b.data(), b.off.data(), b.count(), loff.data(), docs.data(), tf.data(),
                                      static_cast<std::int64_t>(docs.size()), &total));
            if (total <= static_cast<std::int64_t>(docs.size())) break;
            docs.resize(static_cast<std::size_t>(total));
            tf.resize(static_cast<std::size_t>(total));
        }
        return pairs(loff, docs, tf);
    }
    // per pattern the min(k, df) documents with the most occurrences as (doc, tf) pairs, by tf descending and then by document id
    // ascending; 1 <= k <= SA_AMD_DOC_TOPK_MAX
    std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> top_k(const std::vector<std::string> &patterns, std::int32_t k) const
    {
        if (k < 1 || k > SA_AMD_DOC_TOPK_MAX) throw std::invalid_argument("k must be in 1 .. SA_AMD_DOC_TOPK_MAX");
        const Batch b(patterns);
        std::vector<std::int64_t> toff(patterns.size() + 1);
        std::vector<std::uint32_t> docs(patterns.size() * static_cast<std::size_t>(k) + 1), tf(docs.size());
        check(sa_amd_index_doc_topk(ix_, b.data(), b.off.data(), b.count(), k, toff.data(), docs.data(), tf.data()));
        return pairs(toff, docs, tf);
    }
    // the duplicate spans [start, end) that respect the document boundaries (suffix_array_amd.h, "Document-aware duplicate
    // spans"): a window of min_len bytes counts only inside its document.  mode: SA_AMD_REPEATS_ALL / _KEEP_FIRST; scope:
    // SA_AMD_DOCREP_ANY / _OTHER.  doc_bytes != nullptr: resized to one entry per document, the covered bytes inside it.
    std::vector<std::pair<std::uint32_t, std::uint32_t>> repeat_spans(std::int32_t min_len, std::int32_t mode = SA_AMD_REPEATS_KEEP_FIRST,
                                                                      std::int32_t scope = SA_AMD_DOCREP_OTHER,
                                                                      std::vector<std::uint32_t> *doc_bytes = nullptr) const
    {
        const std::int64_t cap = sa_amd_repeat_spans_bound(static_cast<std::int32_t>(n_), min_len);
        if (cap < 0) throw std::invalid_argument("min_len must be at least 1");
        std::vector<std::uint32_t> flat(2 * static_cast<std::size_t>(cap) + 2);
        if (doc_bytes) doc_bytes->assign(ndocs_, 0u);
        std::int64_t count = 0;
        check(sa_amd_index_doc_repeat_spans(ix_, min_len, mode, scope, flat.data(), cap, &count, doc_bytes ? doc_bytes->data() : nullptr));
        std::vector<std::pair<std::uint32_t, std::uint32_t>> out(static_cast<std::size_t>(count < cap ? count : cap));
        for (std::size_t i = 0; i < out.size(); ++i) out[i] = { flat[2 * i], flat[2 * i + 1] };
        return out;
    }
    // the repeated substrings with their document frequency (suffix_array_amd.h, "Repeated substrings with their document
    // frequency"): the rows of suffix_array::repeated_substrings with df, the number of distinct documents an occurrence starts
    // in.  A node is selected when that function's filter holds and df >= min_docs; order SA_AMD_SUBSTR_BY_DOCS ranks by df.
    struct DocSubstring {
        std::uint32_t lo, count, depth, parent;
        std::uint32_t pos;                                        // sa[lo]: where the substring can be read
        std::uint32_t df;
        bool operator==(const DocSubstring &o) const
        {
            return lo == o.lo && count == o.count && depth == o.depth && parent == o.parent && pos == o.pos && df == o.df;
        }
        bool operator!=(const DocSubstring &o) const { return !(*this == o); }
    };
    std::vector<DocSubstring> repeated_substrings(std::int32_t min_len = 1, std::int32_t max_len = 0, std::int32_t min_count = 2,
                                                  std::int64_t min_docs = 1, std::int32_t order = SA_AMD_SUBSTR_ALL, std::int64_t k = 0) const
    {
        const sa_amd_doc_substr_query q = { min_len, max_len, min_count, order, k, min_docs };
        std::int64_t cap = sa_amd_substrings_bound(static_cast<std::int32_t>(n_));
        if (order != SA_AMD_SUBSTR_ALL && k >= 1 && k < cap) cap = k;
        std::vector<std::uint32_t> flat(static_cast<std::size_t>(cap) * 4 + 4), df(static_cast<std::size_t>(cap) + 1), pos(df.size());
        std::int64_t total = 0;
        check(sa_amd_index_doc_substrings(ix_, &q, flat.data(), df.data(), pos.data(), cap, &total));
        std::vector<DocSubstring> out(static_cast<std::size_t>(total < cap ? total : cap));
        for (std::size_t i = 0; i < out.size(); ++i) out[i] = { flat[4 * i], flat[4 * i + 1], flat[4 * i + 2], flat[4 * i + 3], pos[i], df[i] };
        return out;
    }
    // what follows a context in the text and how often (suffix_array_amd.h, "n-gram and infinity-gram queries"): [lo, hi) is the
    // context's match range, at_end says that the context is a suffix of the text, next holds the (byte, count) pairs with a
    // non-zero count in ascending byte order.  The counts and at_end sum to hi - lo.
    struct NextBytes {
        std::uint32_t lo = 0, hi = 0;
        bool at_end = false;
        std::vector<std::pair<std::uint8_t, std::uint32_t>> next;
    };
    // the same for the longest suffix of a prompt that occurs at least min_count times: suffix_len is its length
    struct Infgram : NextBytes {
        std::uint32_t suffix_len = 0;
    };
    std::vector<NextBytes> next_bytes(const std::vector<std::string> &patterns) const
    {
        std::vector<NextBytes> out(patterns.size());
        ngram(patterns, false, 1, 0, out, nullptr);
        return out;
    }
    // max_len <= 0: no cap on the suffix length.  A suffix of length 0 (the byte histogram of the text) always qualifies.
    std::vector<Infgram> infgram(const std::vector<std::string> &prompts, std::int32_t min_count = 1, std::int32_t max_len = 0) const
    {
        if (min_count < 1) throw std::invalid_argument("min_count must be at least 1");
        std::vector<Infgram> out(prompts.size());
        std::vector<std::uint32_t> slen(prompts.size() + 1);
        ngram(prompts, true, min_count, max_len, out, slen.data());
        for (std::size_t q = 0; q < out.size(); ++q) out[q].suffix_len = slen[q];
        return out;
    }
    // a text scored under the infinity-gram model (suffix_array_amd.h, "Scoring a text under the infinity-gram model"): per
    // position of the query the back-off length s, the context's range [lo, hi) and at_end, and [nlo, nhi), the part of that
    // range which the query's byte follows.  count() / total() are the numerator and the denominator of its probability.
    struct Score {
        std::vector<std::uint32_t> s, lo, hi, nlo, nhi;
        std::vector<std::uint8_t> at_end;
        std::size_t size() const { return s.size(); }
        std::uint32_t count(std::size_t j) const { return nhi[j] - nlo[j]; }
        std::uint32_t total(std::size_t j) const { return hi[j] - lo[j] - at_end[j]; }
    };
    // doc_offsets: ndocs + 1 non-decreasing values from 0 to query.size(), or empty for one document; a context never reaches
    // back over the start of its position's document.  1 <= max_len <= SA_AMD_SCORE_MAX_CONTEXT.
    Score infgram_score(const std::string &query, std::int32_t min_count = 1, std::int32_t max_len = SA_AMD_SCORE_MAX_CONTEXT,
                        const std::vector<std::int64_t> &doc_offsets = {}) const
    {
        if (min_count < 1) throw std::invalid_argument("min_count must be at least 1");
        if (max_len < 1 || max_len > SA_AMD_SCORE_MAX_CONTEXT) throw std::invalid_argument("max_len must be 1 .. SA_AMD_SCORE_MAX_CONTEXT");
        const std::size_t m = query.size();
        Score r;
        r.s.resize(m + 1); r.lo.resize(m + 1); r.hi.resize(m + 1); r.nlo.resize(m + 1); r.nhi.resize(m + 1); r.at_end.resize(m + 1);
        check(sa_amd_index_infgram_score(ix_, reinterpret_cast<const std::uint8_t *>(query.data()), static_cast<std::int64_t>(m),
                                         doc_offsets.empty() ? nullptr : doc_offsets.data(),
                                         doc_offsets.empty() ? 0 : static_cast<std::int64_t>(doc_offsets.size()) - 1, min_count, max_len, r.s.data(),
                                         r.lo.data(), r.hi.data(), r.at_end.data(), r.nlo.data(), r.nhi.data()));
        r.s.resize(m); r.lo.resize(m); r.hi.resize(m); r.nlo.resize(m); r.nhi.resize(m); r.at_end.resize(m);
        return r;
    }

private:
    template <class Row>
    void ngram(const std::vector<std::string> &patterns, bool backoff, std::int32_t min_count, std::int32_t max_len, std::vector<Row> &out,
               std::uint32_t *slen) const
    {
        const Batch b(patterns);
        const std::size_t c = patterns.size();
        std::vector<std::uint32_t> lo(c + 1), hi(c + 1), counts(1 << 12);
        std::vector<std::uint8_t> ae(c + 1), bytes(1 << 12);
        std::vector<std::int64_t> loff(c + 1);
        std::int64_t total = 0;
        for (;;) {
            const std::int64_t cap = static_cast<std::int64_t>(bytes.size());
            if (backoff)
                check(sa_amd_index_infgram(ix_, b.data(), b.off.data(), b.count(), min_count, max_len, slen, lo.data(), hi.data(), ae.data(),
                                           loff.data(), bytes.data(), counts.data(), cap, &total));
            else
                check(sa_amd_index_next_bytes(ix_, b.data(), b.off.data(), b.count(), lo.data(), hi.data(), ae.data(), loff.data(), bytes.data(),
                                              counts.data(), cap, &total));
            if (total <= cap) break;
            bytes.resize(static_cast<std::size_t>(total));
            counts.resize(static_cast<std::size_t>(total));
        }
        for (std::size_t q = 0; q < c; ++q) {
            out[q].lo = lo[q]; out[q].hi = hi[q]; out[q].at_end = ae[q] != 0;
            for (std::int64_t e = loff[q]; e < loff[q + 1]; ++e)
                out[q].next.emplace_back(bytes[static_cast<std::size_t>(e)], counts[static_cast<std::size_t>(e)]);
        }
    }
    struct Batch {
        std::string bytes;
        std::vector<std::int64_t> off;
        explicit Batch(const std::vector<std::string> &patterns) : off(patterns.size() + 1, 0)
        {
            for (std::size_t q = 0; q < patterns.size(); ++q) { bytes += patterns[q]; off[q + 1] = static_cast<std::int64_t>(bytes.size()); }
        }
        const std::uint8_t *data() const { return reinterpret_cast<const std::uint8_t *>(bytes.data()); }
        std::int32_t count() const { return static_cast<std::int32_t>(off.size() - 1); }
    };
    static std::vector<std::string> all_patterns(const std::vector<std::vector<Clause>> &queries)
    {
        std::vector<std::string> out;
        for (const auto &query : queries) for (const auto &c : query) out.insert(out.end(), c.any.begin(), c.any.end());
        return out;
    }
    struct Queries {                                              // the layout of sa_amd_index_doc_match
        Batch b;
        std::vector<std::int32_t> coff, qoff;
        std::vector<std::uint8_t> flags;
        explicit Queries(const std::vector<std::vector<Clause>> &queries) : b(all_patterns(queries)), coff(1, 0), qoff(1, 0)
        {
            for (const auto &query : queries) {
                for (const auto &c : query) {
                    coff.push_back(coff.back() + static_cast<std::int32_t>(c.any.size()));
                    flags.push_back(c.negate ? 1 : 0);
                }
                qoff.push_back(static_cast<std::int32_t>(flags.size()));
            }
            flags.push_back(0);                                   // (never an empty buffer)
        }
        std::int32_t clauses() const { return static_cast<std::int32_t>(coff.size() - 1); }
        std::int32_t count() const { return static_cast<std::int32_t>(qoff.size() - 1); }
    };
    static std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> pairs(const std::vector<std::int64_t> &off, const std::vector<std::uint32_t> &docs,
                                                                                    const std::vector<std::uint32_t> &tf)
    {
        std::vector<std::vector<std::pair<std::uint32_t, std::uint32_t>>> out(off.size() - 1);
        for (std::size_t q = 0; q < out.size(); ++q)
            for (std::int64_t e = off[q]; e < off[q + 1]; ++e) out[q].emplace_back(docs[static_cast<std::size_t>(e)], tf[static_cast<std::size_t>(e)]);
        return out;
    }
    static void check(std::int32_t rc)
    {
        if (rc == SA_AMD_EINVAL) throw std::invalid_argument("suffix_array_amd: invalid argument");
        if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    }
    sa_amd_index *ix_ = nullptr;
    std::size_t n_ = 0, ndocs_ = 0;
};

// The entry points of one token width (suffix_array_amd.h): what TokenIndex and TokenIndex32 differ in.
struct TokenAbi16 {
    using Token = std::uint16_t;
    using Handle = sa_amd_tok_index;
    static constexpr std::size_t max_tokens = MAX_LENGTH / 2;
    static constexpr auto create = sa_amd_tok_index_create;
    static constexpr auto destroy = sa_amd_tok_index_destroy;
    static constexpr auto sa = sa_amd_tok_index_sa;
    static constexpr auto search = sa_amd_tok_index_search;
    static constexpr auto next_tokens = sa_amd_tok_index_next_tokens;
    static constexpr auto infgram = sa_amd_tok_index_infgram;
    static constexpr auto infgram_score = sa_amd_tok_index_infgram_score;
    static constexpr auto set_documents = sa_amd_tok_index_set_documents;
    static constexpr auto set_documents_by_separator = sa_amd_tok_index_set_documents_by_separator;
    static constexpr auto doc_offsets = sa_amd_tok_index_doc_offsets;
    static constexpr auto doc_of = sa_amd_tok_index_doc_of;
    static constexpr auto doc_search = sa_amd_tok_index_doc_search;
    static constexpr auto doc_list = sa_amd_tok_index_doc_list;
    static constexpr auto doc_match = sa_amd_tok_index_doc_match;
    static constexpr auto doc_match_list = sa_amd_tok_index_doc_match_list;
};
struct TokenAbi32 {
    using Token = std::uint32_t;
    using Handle = sa_amd_tok32_index;
    static constexpr std::size_t max_tokens = MAX_LENGTH / 3;
    static constexpr auto create = sa_amd_tok32_index_create;
    static constexpr auto destroy = sa_amd_tok32_index_destroy;
    static constexpr auto sa = sa_amd_tok32_index_sa;
    static constexpr auto search = sa_amd_tok32_index_search;
    static constexpr auto next_tokens = sa_amd_tok32_index_next_tokens;
    static constexpr auto infgram = sa_amd_tok32_index_infgram;
    static constexpr auto infgram_score = sa_amd_tok32_index_infgram_score;
    static constexpr auto set_documents = sa_amd_tok32_index_set_documents;
    static constexpr auto set_documents_by_separator = sa_amd_tok32_index_set_documents_by_separator;
    static constexpr auto doc_offsets = sa_amd_tok32_index_doc_offsets;
    static constexpr auto doc_of = sa_amd_tok32_index_doc_of;
    static constexpr auto doc_search = sa_amd_tok32_index_doc_search;
    static constexpr auto doc_list = sa_amd_tok32_index_doc_list;
    static constexpr auto doc_match = sa_amd_tok32_index_doc_match;
    static constexpr auto doc_match_list = sa_amd_tok32_index_doc_match_list;
};

// EXTENSION (not in the reference): a token text and its suffix array resident on the device.  Tokens compare as unsigned
// values; every length, position and offset is in tokens.
//   TokenIndex    16-bit tokens (sa_amd_tok_index; suffix_array_amd.h, "Texts over a 16-bit token alphabet")
//   TokenIndex32  token ids below 2^24 in std::uint32_t (sa_amd_tok32_index; suffix_array_amd_tok32.h): an id of
//                 2^24 or more in the text, a pattern, a prompt or a query throws std::runtime_error (SA_AMD_ERANGE)
template <class Abi>
class BasicTokenIndex {
public:
    using Token = typename Abi::Token;
    using Tokens = std::vector<Token>;
    // sa == nullptr: the suffix array is built on the device and never downloaded; a supplied one (n + 1 entries) is range-checked
    BasicTokenIndex(const Token *t, std::size_t n, const std::uint32_t *sa = nullptr)
    {
        if (n > Abi::max_tokens) throw std::logic_error("assertion failed: t.len() <= the longest token text");
        check(Abi::create(t, static_cast<std::int32_t>(n), sa, &ix_));
        n_ = n;
    }
    BasicTokenIndex(const BasicTokenIndex &) = delete;
    BasicTokenIndex &operator=(const BasicTokenIndex &) = delete;
    ~BasicTokenIndex() { Abi::destroy(ix_); }

    std::size_t len() const { return n_; }
    // the token suffix array: n + 1 entries, entry 0 is n
    std::vector<std::uint32_t> sa() const
    {
        std::vector<std::uint32_t> out(n_ + 1);
        check(Abi::sa(ix_, out.data()));
        return out;
    }
    // per pattern its match range [lo, hi) in the token suffix array; lo == hi where it does not occur
    std::vector<std::pair<std::uint32_t, std::uint32_t>> search(const std::vector<Tokens> &patterns) const
    {
        const Batch b(patterns);
        std::vector<std::uint32_t> lo(patterns.size() + 1), hi(patterns.size() + 1);
        check(Abi::search(ix_, b.toks.data(), b.off.data(), b.count(), nullptr, lo.data(), hi.data()));
        std::vector<std::pair<std::uint32_t, std::uint32_t>> out(patterns.size());
        for (std::size_t q = 0; q < out.size(); ++q) out[q] = { lo[q], hi[q] };
        return out;
    }
    // occurrences of every pattern (the empty pattern has n + 1), and whether it occurs at all
    std::vector<std::uint32_t> count(const std::vector<Tokens> &patterns) const
    {
        const auto r = search(patterns);
        std::vector<std::uint32_t> out(r.size());
        for (std::size_t q = 0; q < out.size(); ++q) out[q] = r[q].second - r[q].first;
        return out;
    }
    std::vector<bool> contains(const std::vector<Tokens> &patterns) const
    {
        const auto r = search(patterns);
        std::vector<bool> out(r.size());
        for (std::size_t q = 0; q < out.size(); ++q) out[q] = r[q].second > r[q].first;
        return out;
    }
    // what follows a context and how often: next holds the (token, count) pairs with a non-zero count in ascending token order;
    // the counts and at_end sum to hi - lo
    struct NextTokens {
        std::uint32_t lo = 0, hi = 0;
        bool at_end = false;
        std::vector<std::pair<Token, std::uint32_t>> next;
    };
    // the same for the longest suffix of a prompt that occurs at least min_count times: suffix_len is its length in tokens
    struct Infgram : NextTokens {
        std::uint32_t suffix_len = 0;
    };
    std::vector<NextTokens> next_tokens(const std::vector<Tokens> &patterns) const
    {
        std::vector<NextTokens> out(patterns.size());
        ngram(patterns, false, 1, 0, out, nullptr);
        return out;
    }
    // max_len <= 0: no cap on the suffix length.  A suffix of length 0 (the token histogram of the text) always qualifies.
    std::vector<Infgram> infgram(const std::vector<Tokens> &prompts, std::int32_t min_count = 1, std::int32_t max_len = 0) const
    {
        if (min_count < 1) throw std::invalid_argument("min_count must be at least 1");
        std::vector<Infgram> out(prompts.size());
        std::vector<std::uint32_t> slen(prompts.size() + 1);
        ngram(prompts, true, min_count, max_len, out, slen.data());
        for (std::size_t q = 0; q < out.size(); ++q) out[q].suffix_len = slen[q];
        return out;
    }
    // a token text scored under the infinity-gram model (suffix_array_amd.h, "Scoring a token text under the infinity-gram
    // model"): DocumentIndex::infgram_score with tokens in place of bytes -- s, max_len and doc_offsets are in tokens, the ranges
    // are slots of the token suffix array, [nlo, nhi) is the part of the context's range which the query's token follows.
    using Score = DocumentIndex::Score;
    Score infgram_score(const Tokens &query, std::int32_t min_count = 1, std::int32_t max_len = SA_AMD_SCORE_MAX_CONTEXT,
                        const std::vector<std::int64_t> &doc_offsets = {}) const
    {
        if (min_count < 1) throw std::invalid_argument("min_count must be at least 1");
        if (max_len < 1 || max_len > SA_AMD_SCORE_MAX_CONTEXT) throw std::invalid_argument("max_len must be 1 .. SA_AMD_SCORE_MAX_CONTEXT");
        const std::size_t m = query.size();
        Score r;
        r.s.resize(m + 1); r.lo.resize(m + 1); r.hi.resize(m + 1); r.nlo.resize(m + 1); r.nhi.resize(m + 1); r.at_end.resize(m + 1);
        check(Abi::infgram_score(ix_, m ? query.data() : nullptr, static_cast<std::int64_t>(m),
                                 doc_offsets.empty() ? nullptr : doc_offsets.data(),
                                 doc_offsets.empty() ? 0 : static_cast<std::int64_t>(doc_offsets.size()) - 1, min_count, max_len,
                                 r.s.data(), r.lo.data(), r.hi.data(), r.at_end.data(), r.nlo.data(), r.nhi.data()));
        r.s.resize(m); r.lo.resize(m); r.hi.resize(m); r.nlo.resize(m); r.nhi.resize(m); r.at_end.resize(m);
        return r;
    }

    // ---- document collections (sa_amd_tokdocs.h): the methods of DocumentIndex with tokens for bytes ----

    // offsets: ndocs + 1 non-decreasing values from 0 to len(), in tokens.  Replaces the collection; malformed offsets throw
    // std::invalid_argument and leave the previous one in place.  -> ndocs
    std::size_t set_documents(const std::vector<std::uint32_t> &offsets)
    {
        if (offsets.size() < 2) throw std::invalid_argument("document offsets: ndocs + 1 values from 0 to n");
        check(Abi::set_documents(ix_, offsets.data(), static_cast<std::int64_t>(offsets.size()) - 1));
        return offsets.size() - 1;
    }
    // every occurrence of `separator` ends a document and belongs to it; found on the device in the resident text.  -> ndocs
    std::size_t set_documents_by_separator(Token separator)
    {
        std::int64_t nd = 0;
        check(Abi::set_documents_by_separator(ix_, separator, &nd));
        return static_cast<std::size_t>(nd);
    }
    // documents of the collection in effect, as the library holds it (no copy is kept here); 0 before a collection was set
    std::size_t ndocs() const
    {
        std::int64_t nd = 0;
        const std::int32_t rc = Abi::doc_offsets(ix_, nullptr, 0, &nd);
        if (rc == SA_AMD_EINVAL) return 0;
        check(rc);
        return static_cast<std::size_t>(nd);
    }
    // the collection in effect: ndocs + 1 offsets in tokens
    std::vector<std::uint32_t> doc_offsets() const
    {
        std::int64_t nd = 0;
        check(Abi::doc_offsets(ix_, nullptr, 0, &nd));
        std::vector<std::uint32_t> out(static_cast<std::size_t>(nd) + 1);
        check(Abi::doc_offsets(ix_, out.data(), static_cast<std::int64_t>(out.size()), &nd));
        if (static_cast<std::size_t>(nd) + 1 > out.size()) throw std::runtime_error("suffix_array_amd: the collection was replaced during doc_offsets");
        out.resize(static_cast<std::size_t>(nd) + 1);
        return out;
    }
    // the document of every token position; SA_AMD_DOC_NONE for positions >= len()
    std::vector<std::uint32_t> doc_of(const std::vector<std::uint32_t> &positions) const
    {
        std::vector<std::uint32_t> out(positions.size());
        check(Abi::doc_of(ix_, positions.data(), static_cast<std::int64_t>(positions.size()), out.data()));
        return out;
    }
    // per pattern (occ, df): occurrences, and the number of distinct documents an occurrence starts in
    std::vector<std::pair<std::uint32_t, std::uint32_t>> doc_search(const std::vector<Tokens> &patterns) const
    {
        const Batch b(patterns);
        std::vector<std::uint32_t> occ(patterns.size() + 1), df(patterns.size() + 1);
        check(Abi::doc_search(ix_, b.toks.data(), b.off.data(), b.count(), occ.data(), df.data()));
        std::vector<std::pair<std::uint32_t, std::uint32_t>> out(patterns.size());
        for (std::size_t q = 0; q < out.size(); ++q) out[q] = { occ[q], df[q] };
        return out;
    }
    // per pattern the distinct documents it occurs in, in slot order
    std::vector<std::vector<std::uint32_t>> doc_list(const std::vector<Tokens> &patterns) const
    {
        const Batch b(patterns);
        return listing(patterns.size(), [&](std::int64_t *loff, std::uint32_t *docs, std::int64_t cap, std::int64_t *total) {
            return Abi::doc_list(ix_, b.toks.data(), b.off.data(), b.count(), loff, docs, cap, total);
        });
    }
    // Boolean document queries: a query is the AND of its clauses, a clause the OR of its token patterns, negated where `negate`
    // is set.  -> per query the number of documents it holds in; match_list: the documents, in ascending document id.
    using Clause = BasicClause<Tokens>;
    std::vector<std::uint32_t> match(const std::vector<std::vector<Clause>> &queries) const
    {
        const Queries q(queries);
        std::vector<std::uint32_t> df(queries.size() + 1);
        check(Abi::doc_match(ix_, q.b.toks.data(), q.b.off.data(), q.b.count(), q.coff.data(), q.flags.data(), q.clauses(), q.qoff.data(), q.count(),
                             df.data(), nullptr));
        df.resize(queries.size());
        return df;
    }
    std::vector<std::vector<std::uint32_t>> match_list(const std::vector<std::vector<Clause>> &queries) const
    {
        const Queries q(queries);
        return listing(queries.size(), [&](std::int64_t *loff, std::uint32_t *docs, std::int64_t cap, std::int64_t *total) {
            return Abi::doc_match_list(ix_, q.b.toks.data(), q.b.off.data(), q.b.count(), q.coff.data(), q.flags.data(), q.clauses(), q.qoff.data(),
                                       q.count(), loff, docs, cap, total);
        });
    }

private:
    struct Batch {
        Tokens toks;
        std::vector<std::int64_t> off;
        explicit Batch(const std::vector<Tokens> &patterns) : off(patterns.size() + 1, 0)
        {
            for (std::size_t q = 0; q < patterns.size(); ++q) {
                toks.insert(toks.end(), patterns[q].begin(), patterns[q].end());
                off[q + 1] = static_cast<std::int64_t>(toks.size());
            }
            if (toks.empty()) toks.push_back(0);       // (never a NULL pattern pointer)
        }
        std::int32_t count() const { return static_cast<std::int32_t>(off.size() - 1); }
    };
    static std::vector<Tokens> all_patterns(const std::vector<std::vector<Clause>> &queries)
    {
        std::vector<Tokens> out;
        for (const auto &query : queries) for (const auto &c : query) out.insert(out.end(), c.any.begin(), c.any.end());
        return out;
    }
    struct Queries {                                              // the layout of sa_amd_index_doc_match
        Batch b;
        std::vector<std::int32_t> coff, qoff;
        std::vector<std::uint8_t> flags;
        explicit Queries(const std::vector<std::vector<Clause>> &queries) : b(all_patterns(queries)), coff(1, 0), qoff(1, 0)
        {
            for (const auto &query : queries) {
                for (const auto &c : query) {
                    coff.push_back(coff.back() + static_cast<std::int32_t>(c.any.size()));
                    flags.push_back(c.negate ? 1 : 0);
                }
                qoff.push_back(static_cast<std::int32_t>(flags.size()));
            }
            flags.push_back(0);                                   // (never an empty buffer)
        }
        std::int32_t clauses() const { return static_cast<std::int32_t>(coff.size() - 1); }
        std::int32_t count() const { return static_cast<std::int32_t>(qoff.size() - 1); }
    };
    // a listing of `rows` rows: asked for again with the capacity the first call reported where it did not fit
    template <class Call>
    static std::vector<std::vector<std::uint32_t>> listing(std::size_t rows, Call call)
    {
        std::vector<std::int64_t> loff(rows + 1);
        std::vector<std::uint32_t> docs(1 << 16);
        std::int64_t total = 0;
        for (;;) {
            check(call(loff.data(), docs.data(), static_cast<std::int64_t>(docs.size()), &total));
            if (total <= static_cast<std::int64_t>(docs.size())) break;
            docs.resize(static_cast<std::size_t>(total));
        }
        std::vector<std::vector<std::uint32_t>> out(rows);
        for (std::size_t q = 0; q < rows; ++q) out[q].assign(docs.begin() + loff[q], docs.begin() + loff[q + 1]);
        return out;
    }
    template <class Row>
    void ngram(const std::vector<Tokens> &patterns, bool backoff, std::int32_t min_count, std::int32_t max_len, std::vector<Row> &out,
               std::uint32_t *slen) const
    {
        const Batch b(patterns);
        const std::size_t c = patterns.size();
        std::vector<std::uint32_t> lo(c + 1), hi(c + 1), counts(1 << 12);
        std::vector<std::uint8_t> ae(c + 1);
        Tokens toks(1 << 12);
        std::vector<std::int64_t> loff(c + 1);
        std::int64_t total = 0;
        for (;;) {
            const std::int64_t cap = static_cast<std::int64_t>(toks.size());
            if (backoff)
                check(Abi::infgram(ix_, b.toks.data(), b.off.data(), b.count(), min_count, max_len, slen, lo.data(), hi.data(), ae.data(),
                                   loff.data(), toks.data(), counts.data(), cap, &total));
            else
                check(Abi::next_tokens(ix_, b.toks.data(), b.off.data(), b.count(), lo.data(), hi.data(), ae.data(), loff.data(),
                                       toks.data(), counts.data(), cap, &total));
            if (total <= cap) break;
            toks.resize(static_cast<std::size_t>(total));
            counts.resize(static_cast<std::size_t>(total));
        }
        for (std::size_t q = 0; q < c; ++q) {
            out[q].lo = lo[q]; out[q].hi = hi[q]; out[q].at_end = ae[q] != 0;
            for (std::int64_t e = loff[q]; e < loff[q + 1]; ++e)
                out[q].next.emplace_back(toks[static_cast<std::size_t>(e)], counts[static_cast<std::size_t>(e)]);
        }
    }
    static void check(std::int32_t rc)
    {
        if (rc == SA_AMD_EINVAL) throw std::invalid_argument("suffix_array_amd: invalid argument");
        if (rc != SA_AMD_OK) throw std::runtime_error(std::string("suffix_array_amd: ") + sa_amd_strerror(rc));
    }
    typename Abi::Handle *ix_ = nullptr;
    std::size_t n_ = 0;
};

using TokenIndex = BasicTokenIndex<TokenAbi16>;
using TokenIndex32 = BasicTokenIndex<TokenAbi32>;

}  // namespace suffix_array
