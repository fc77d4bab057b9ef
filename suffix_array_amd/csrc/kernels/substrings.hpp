// kernels/substrings.hpp -- repeated substrings: the internal nodes of the suffix tree from the LCP array, filtered, in slot order
// or the best k of them.  Part of the MI355X-native suffix-array engine (gfx950 / CDNA4, wave64).
//
// SA and LCP are in the layout of sa_amd_saca_u8 and sa_amd_lcp: n + 1 entries ("slots" 0 .. n here), LCP[0] = LCP[1] = 0.
//   A slot i, 2 <= i <= n, is a REPRESENTATIVE when d = LCP[i] > 0 and the nearest j < i with LCP[j] <= d has LCP[j] < d; that j
//   is lo (lo >= 1).  hi = the nearest j > i with LCP[j] < d, n + 1 when there is none.
//   Its NODE is the row (lo, count = hi - lo >= 2, depth = d, parent = max(LCP[lo], LCP[hi]) < d, LCP[n + 1] read as 0): the
//   substring T[SA[lo] .. SA[lo] + depth) occurs at exactly SA[lo .. lo + count), and so does every prefix longer than parent.
//   Among the slots of one node (equal values with nothing smaller between them) only the leftmost is a representative: every
//   other one meets an equal value first on its left.
//   Query (min_len, max_len, min_count): a node is SELECTED when depth >= min_len, (max_len == 0 or parent < max_len) and
//   count >= min_count; len = depth, or min(depth, max_len) when max_len != 0.
//
// Neighbour slots: stage 1 of kernels/lz.hpp over LCP[0 .. n] -- k_lz_tile<true>, k_lz_level, k_lz_far<false, true> --, the
// left side asking for "< d + 1" (values are below 2^31), the right side for "< d".  The minima are exact whatever the values,
// so a block with a minimum below the query value has a child with one: equal values change nothing in the descent.
//   k_sub_nodes<0>   per slot: representative, node, filter; selected nodes per tile; the four counters and the largest key
//   k_rep_sum_spine  running sum of the tiles' counts
//   k_sub_nodes<1>   ORDER_ALL: row c, c < capacity, to rows[4 c ..] and SA[lo] to pos[c], in slot order;
//                    ranked: candidate c = (key, slot) to ckeys[c], cslots[c], in slot order
// Exact top-k of the candidates without sorting them (ranked orders; key = count, len or count * len, 64 bits):
//   k_sub_hist       radix select: counts of one 8-bit digit over the candidates whose higher bits equal the prefix found so far
//   k_sub_cut<0/1>   every candidate with key >= above is kept, and the first `need` in slot order with at_cut <= key < above:
//                    counts per tile of both kinds, two running sums, then (~key, candidate index) in slot order -- the place
//                    of a kept candidate is (above-kind in front) + min(cut-kind in front, need), so one pair of sums does
//   sort_pairs       on exactly min(k, selected) pairs, key bits [0, width of the largest key): stable, so equal keys stay in
//                    slot order
//   k_sub_gather     row and pos of sorted pair r, r < capacity
// DF = true (kernels/doc_substrings.hpp): the node pass and the gather also read the scanned table E of
// the document pairs -- df = count - (E[hi] - E[lo + 1]) --, filter by df >= min_docs, rank by df under SUB_ORDER_DOCS and
// write df beside the rows.  DF = false is the arithmetic of section 19, unchanged.
#pragma once
#include "lz.hpp"

namespace sa {

constexpr int SUB_ORDER_ALL = 0, SUB_ORDER_COUNT = 1, SUB_ORDER_LENGTH = 2, SUB_ORDER_COVER = 3;
constexpr int SUB_ORDER_DOCS = 4;               // DF = true only: key = df
constexpr int SUB_HIST_THREADS = 256;

// control words (uint64) at byte 128 of the LCP control slab; the first three are stage 1's (LZ_C_UNRES, LZ_C_HSTEPS, LZ_C_HMAX)
constexpr int SUB_C_NODES = 3, SUB_C_SELECTED = 4, SUB_C_DALL = 5, SUB_C_DSEL = 6, SUB_C_MAXKEY = 7, SUB_C_TOTAL = 8, SUB_C_ABOVE = 9,
              SUB_C_ATCUT = 10, SUB_C_WORDS = 11;
static_assert(LZ_C_HMAX < SUB_C_NODES, "stage 1 counts into the same slab");

struct SubQuery { uint32_t min_len, max_len, min_count; int order; };
struct SubNode { uint32_t lo, count, depth, parent; };
// DF = true: E (n + 2 entries), the filter, the df column (may be null) and the DSUB_C_* control words; unused when DF = false
struct SubDf { const uint32_t *E; uint32_t min_docs; uint32_t *df; unsigned long long *ctl; };
constexpr int DSUB_C_DFSUM = 0, DSUB_C_MAXDF = 1;       // the node pass's two of the DSUB_C_* words (kernels/doc_substrings.hpp)

// the node of slot i when i is a representative (every index read is checked against the tables first)
__device__ __forceinline__ bool sub_node(const uint32_t *__restrict__ LCP, const uint32_t *__restrict__ psl, const uint32_t *__restrict__ nsl,
                                         int64_t n, int64_t i, SubNode &nd)
{
    if (i < 2 || i > n) return false;
    const uint32_t d = LCP[i];
    if (d == 0u) return false;
    const uint32_t pl = psl[i];
    if ((int64_t)pl >= i) return false;                       // (LZ_NONE: cannot be, LCP[1] = 0)
    const uint32_t a = LCP[pl];
    if (!(a < d)) return false;                               // an equal value first: the node's representative is further left
    const uint32_t nr = nsl[i];
    const int64_t hi = (int64_t)nr <= n ? (int64_t)nr : n + 1;
    const uint32_t b = hi <= n ? LCP[hi] : 0u;
    nd.lo = pl;
    nd.count = (uint32_t)(hi - (int64_t)pl);
    nd.depth = d;
    nd.parent = a > b ? a : b;
    return true;
}

__device__ __forceinline__ bool sub_selected(const SubNode &nd, const SubQuery &q, uint32_t &len)
{
    len = q.max_len == 0u || nd.depth < q.max_len ? nd.depth : q.max_len;
    return nd.depth >= q.min_len && (q.max_len == 0u || nd.parent < q.max_len) && nd.count >= q.min_count;
}

__device__ __forceinline__ unsigned long long sub_key(const SubNode &nd, uint32_t len, int order)
{
    return order == SUB_ORDER_COUNT ? (unsigned long long)nd.count
         : order == SUB_ORDER_LENGTH ? (unsigned long long)len : (unsigned long long)nd.count * len;
}

// distinct documents among the node's slots: its count less the pairs counted strictly inside it.  sub_node has checked
// lo + 1 <= hi = lo + count <= n + 1, and E has n + 2 entries.
__device__ __forceinline__ uint32_t sub_df(const SubNode &nd, const uint32_t *__restrict__ E)
{
    return nd.count - (E[nd.lo + nd.count] - E[nd.lo + 1u]);
}

// WRITE = 0: cnt[tile] = selected nodes of the tile; nodes, selected, the two sums and the largest key to ctl.
// WRITE = 1: cnt holds the selected nodes in front of every tile (k_rep_sum_spine); ORDER_ALL: the first `capacity` rows (and
// pos, when not null); ranked: every candidate's key and slot.
// DF: selected also needs df >= d.min_docs; the sum and the largest df of the selected nodes to d.ctl; df beside the rows.
template <int WRITE, bool DF = false>
__global__ __launch_bounds__(REP_THREADS) void k_sub_nodes(const uint32_t *__restrict__ LCP, const uint32_t *__restrict__ psl,
                                                            const uint32_t *__restrict__ nsl, const uint32_t *__restrict__ SA, int64_t n, SubQuery q,
                                                            uint32_t *__restrict__ cnt, uint32_t *__restrict__ rows, uint32_t *__restrict__ pos,
                                                            int64_t capacity, unsigned long long *__restrict__ ckeys, uint32_t *__restrict__ cslots,
                                                            unsigned long long *__restrict__ ctl, SubDf d)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)t * REP_ITEMS;
    SubNode nd[REP_ITEMS];
    uint32_t dfv[DF ? REP_ITEMS : 1];
    uint32_t bits = 0, dmax = 0;
    unsigned long long nodes = 0, dall = 0, dsel = 0, best = 0, dfs = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        if (!sub_node(LCP, psl, nsl, n, j0 + k, nd[k])) continue;
        uint32_t len;
        bool sel = sub_selected(nd[k], q, len);
        if (DF) {
            dfv[k] = sub_df(nd[k], d.E);
            sel = sel && dfv[k] >= d.min_docs;
        }
        if (sel) bits |= 1u << k;
        if (WRITE == 0) {
            ++nodes;
            dall += nd[k].depth - nd[k].parent;
            if (sel) {
                const uint32_t floor = nd[k].parent > q.min_len - 1u ? nd[k].parent : q.min_len - 1u;
                dsel += len - floor;
                const unsigned long long key = DF && q.order == SUB_ORDER_DOCS ? (unsigned long long)dfv[DF ? k : 0] : sub_key(nd[k], len, q.order);
                best = best > key ? best : key;
                if (DF) { dfs += dfv[k]; dmax = dmax > dfv[k] ? dmax : dfv[k]; }
            }
        }
    }
    uint32_t total;
    const uint32_t ex = block_excl_sum<REP_THREADS>((uint32_t)__popc(bits), lds, &total);
    if (WRITE == 0) {
        if (t == 0) cnt[blockIdx.x] = total;
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) { const unsigned long long b2 = __shfl_xor(best, o, WAVE); best = best > b2 ? best : b2; }
        if (lane_id() == 0 && best) atomicMax(&ctl[SUB_C_MAXKEY], best);
        lcp_block_add(nodes, &ctl[SUB_C_NODES]);
        lcp_block_add((unsigned long long)__popc(bits), &ctl[SUB_C_SELECTED]);
        lcp_block_add(dall, &ctl[SUB_C_DALL]);
        lcp_block_add(dsel, &ctl[SUB_C_DSEL]);
        if (DF) {
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) { const uint32_t m2 = __shfl_xor(dmax, o, WAVE); dmax = dmax > m2 ? dmax : m2; }
            if (lane_id() == 0 && dmax) atomicMax(&d.ctl[DSUB_C_MAXDF], (unsigned long long)dmax);
            lcp_block_add(dfs, &d.ctl[DSUB_C_DFSUM]);
        }
    } else {
        int64_t c = (int64_t)cnt[blockIdx.x] + ex;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            if (!((bits >> k) & 1u)) continue;
            if (q.order != SUB_ORDER_ALL) {
                uint32_t len;
                (void)sub_selected(nd[k], q, len);
                ckeys[c] = DF && q.order == SUB_ORDER_DOCS ? (unsigned long long)dfv[DF ? k : 0] : sub_key(nd[k], len, q.order);
                cslots[c] = (uint32_t)(j0 + k);
            } else if (c < capacity) {
                rows[4 * c] = nd[k].lo;
                rows[4 * c + 1] = nd[k].count;
                rows[4 * c + 2] = nd[k].depth;
                rows[4 * c + 3] = nd[k].parent;
                if (pos) pos[c] = SA[nd[k].lo];
                if (DF && d.df) d.df[c] = dfv[DF ? k : 0];
            }
            ++c;
        }
    }
}

// hist[d] += candidates with (key >> match_shift) == prefix (match_shift >= 64: all of them) whose digit (key >> shift) & 255 is d
__global__ __launch_bounds__(SUB_HIST_THREADS) void k_sub_hist(const unsigned long long *__restrict__ ckeys, int64_t m, int match_shift,
                                                               unsigned long long prefix, int shift, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * SUB_HIST_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SUB_HIST_THREADS + threadIdx.x; i < m; i += stride) {
        const unsigned long long key = ckeys[i];
        if (match_shift >= 64 || (key >> match_shift) == prefix) atomicAdd(&h[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}
static_assert(SUB_HIST_THREADS == 256, "one thread per bin");

// WRITE = 0: cnt_a[tile] = candidates with key >= above, cnt_e[tile] = those with at_cut <= key < above.
// WRITE = 1: both hold the running sums; a kept candidate goes to place (above-kind in front) + min(cut-kind in front, need).
template <int WRITE>
__global__ __launch_bounds__(REP_THREADS) void k_sub_cut(const unsigned long long *__restrict__ ckeys, int64_t m, unsigned long long above,
                                                          unsigned long long at_cut, int64_t need, uint32_t *__restrict__ cnt_a,
                                                          uint32_t *__restrict__ cnt_e, unsigned long long *__restrict__ skeys,
                                                          uint32_t *__restrict__ svals)
{
    __shared__ uint32_t lds[REP_WAVES + 1];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * REP_TILE + (int64_t)t * REP_ITEMS;
    unsigned long long key[REP_ITEMS];
    uint32_t ba = 0, be = 0;
#pragma unroll
    for (int k = 0; k < REP_ITEMS; ++k) {
        key[k] = 0;
        if (j0 + k >= m) continue;
        key[k] = ckeys[j0 + k];
        if (key[k] >= above) ba |= 1u << k;
        else if (key[k] >= at_cut) be |= 1u << k;
    }
    uint32_t tot_a, tot_e;
    const uint32_t ex_a = block_excl_sum<REP_THREADS>((uint32_t)__popc(ba), lds, &tot_a);
    const uint32_t ex_e = block_excl_sum<REP_THREADS>((uint32_t)__popc(be), lds, &tot_e);
    if (WRITE == 0) {
        if (t == 0) { cnt_a[blockIdx.x] = tot_a; cnt_e[blockIdx.x] = tot_e; }
    } else {
        int64_t a = (int64_t)cnt_a[blockIdx.x] + ex_a, e = (int64_t)cnt_e[blockIdx.x] + ex_e;
#pragma unroll
        for (int k = 0; k < REP_ITEMS; ++k) {
            const bool isa = (ba >> k) & 1u, ise = (be >> k) & 1u;
            if (isa || (ise && e < need)) {
                const int64_t out = a + (e < need ? e : need);
                skeys[out] = ~key[k];
                svals[out] = (uint32_t)(j0 + k);
            }
            a += isa ? 1 : 0;
            e += ise ? 1 : 0;
        }
    }
}

// rows[4 r ..] and pos[r] (when not null) of the sorted pair r, r < count: its value is a candidate index, cslots holds the slot.
// DF: and d.df[r] (when not null).
template <bool DF = false>
__global__ __launch_bounds__(SUB_HIST_THREADS) void k_sub_gather(const uint32_t *__restrict__ svals, int64_t count, int64_t m,
                                                                 const uint32_t *__restrict__ cslots, const uint32_t *__restrict__ LCP,
                                                                 const uint32_t *__restrict__ psl, const uint32_t *__restrict__ nsl,
                                                                 const uint32_t *__restrict__ SA, int64_t n, uint32_t *__restrict__ rows,
                                                                 uint32_t *__restrict__ pos, SubDf d)
{
    const int64_t r = (int64_t)blockIdx.x * SUB_HIST_THREADS + threadIdx.x;
    if (r >= count) return;
    const uint32_t c = svals[r];
    SubNode nd = { 0u, 0u, 0u, 0u };
    const bool ok = (int64_t)c < m && sub_node(LCP, psl, nsl, n, (int64_t)cslots[c], nd);     // (always: the pair came from the candidates)
    rows[4 * r] = nd.lo;
    rows[4 * r + 1] = nd.count;
    rows[4 * r + 2] = nd.depth;
    rows[4 * r + 3] = nd.parent;
    if (pos) pos[r] = ok ? SA[nd.lo] : 0u;
    if (DF && d.df) d.df[r] = ok ? sub_df(nd, d.E) : 0u;
}

}  // namespace sa
