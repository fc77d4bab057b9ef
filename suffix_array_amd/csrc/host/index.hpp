// host/index.hpp -- the device-resident index: the one definition of the type behind the ABI's `sa_amd_index *`
// (include/suffix_array_amd.h), the owner of every allocation that outlives a call ("The index owner").
#pragma once
#include "support.hpp"

// Text and suffix array kept in HBM, and the tables the enabling calls add to them.  Every allocation is a DevBuf of the index's
// own (never the pool's): deleting the index frees them all, in no call that can throw and without a change of device.  A route
// that builds a table allocates it with index_table_alloc, builds it inside a PooledScope and hands it over by move-assignment
// only after the scope's finish() succeeded -- a failed build leaves the index as it was.
extern "C++" {

struct sa_amd_index {
    int device = 0;
    int32_t n = 0;
    uint32_t ndocs = 0;
    sa::DevBuf dT, dSA;
    sa::DevBuf dBkt;       // bucket table once sa_amd_index_buckets has built it (narrows the searches, src/sa.rs:123-161)
    sa::DevBuf dPair;      // LCP table of the search tree once sa_amd_index_enable_lcp has built it (kernels/esa.hpp)
    sa::DevBuf dDocOff;    // document offsets (ndocs + 1 entries) once sa_amd_index_set_documents has taken a collection (kernels/docs.hpp)
    sa::DevBuf dDocPrev;   // per slot: the previous slot of the same document + 1 (n + 1 entries)
    sa::DevBuf dDocSlots;  // the slots 1 .. n ordered by document once sa_amd_index_enable_doc_freq has built them (kernels/doc_tf.hpp)

    // what the kernels receive; nullptr for a table that has not been built
    const uint8_t *text() const { return dT.as<const uint8_t>(); }
    const uint32_t *sa() const { return dSA.as<const uint32_t>(); }
    const uint32_t *bkt() const { return dBkt.as<const uint32_t>(); }
    const uint64_t *pair() const { return dPair.as<const uint64_t>(); }
    const uint32_t *doc_off() const { return dDocOff.as<const uint32_t>(); }
    const uint32_t *doc_prev() const { return dDocPrev.as<const uint32_t>(); }
    const uint32_t *doc_slots() const { return dDocSlots.as<const uint32_t>(); }
};

}  // extern "C++"

namespace sa {

// the allocation of a table that is to outlive the call (DevBuf::alloc clears a refused allocation's error, for every caller)
static inline int32_t index_table_alloc(DevBuf &b, size_t bytes) { return b.alloc(bytes); }

}  // namespace sa
