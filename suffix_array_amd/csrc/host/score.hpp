// host/score.hpp -- scoring a query text under the infinity-gram model against a device-resident index (kernels/score.hpp,
// DESIGN.md sections 22 and 24): argument checks, work-block layout, the two passes, the host-pointer route.  Written once over
// the index type: the byte index (sa_amd_index, Sym = uint8_t) and the token index (sa_amd_tok_index, Sym = uint16_t) differ in
// the symbol type of text(), in the tables (the token index has none) and in the statistics block they write.
#pragma once
#include "match.hpp"
#include "ngram.hpp"
#include "../kernels/score.hpp"

namespace sa {

static thread_local sa_amd_score_stats g_last_score_stats;
static thread_local sa_amd_tok_score_stats g_last_tok_score_stats;     // of the token route: neither the one above nor sa_amd_tok_stats is touched
static thread_local int32_t g_score_cap = -1;          // sa_amd_score_set_group_cap of the calling thread (-1: SCORE_CAP_DEFAULT)

// layout of the work block: control words | the document offsets (ndocs + 1) | the long list: position, range lo, range hi (m each)
struct ScoreLayout { size_t ctl, off, list, lo, hi, bytes; };
static ScoreLayout score_layout(int64_t m, int64_t ndocs)
{
    ScoreLayout L;
    size_t off = 0;
    auto take = [&](size_t b) { const size_t o = off; off = align_up(off + b, 256); return o; };
    L.ctl = take(256);
    L.off = take(((size_t)ndocs + 1) * 8);
    L.list = take(((size_t)m + 1) * 4);
    L.lo = take(((size_t)m + 1) * 4);
    L.hi = take(((size_t)m + 1) * 4);
    L.bytes = off;
    return L;
}
static_assert(SC_W_COUNT * 8 <= 256, "control slab");

// what can be refused without a device: q_off == nullptr is one document [0, m) (ndocs is ignored then)
static bool score_args_valid(int64_t m, const int64_t *q_off, int64_t ndocs, int32_t min_count, int32_t max_len)
{
    if (m < 0 || m > (int64_t)SA_AMD_MAX_LENGTH || min_count < 1 || max_len < 1 || max_len > SA_AMD_SCORE_MAX_CONTEXT) return false;
    if (!q_off) return true;
    if (ndocs < 0 || ndocs > (int64_t)SA_AMD_MAX_LENGTH || q_off[0] != 0 || q_off[ndocs] != m) return false;
    for (int64_t d = 0; d < ndocs; ++d)
        if (q_off[d + 1] < q_off[d]) return false;
    return true;
}

// dQ: m symbols on the index's device (any address aligned to Sym); the outputs: m entries each on that device, any of them
// nullptr; q_off: HOST offsets, checked by the caller; dWork: score_layout(m, ndocs).bytes, 256-byte aligned.  Blocks until
// done.  last / compared: the calling thread's statistics block of this index type and its compared-symbols field.
template <typename Index, typename Sym, typename Stats>
static int score_device(const Index &ix, const Sym *dQ, int64_t m, const int64_t *q_off, int64_t ndocs, int32_t min_count, int32_t max_len,
                        const ScoreOut &out, void *dWork, int64_t work_bytes, hipStream_t st, Stats &last, int64_t Stats::*compared)
{
    static_assert(std::is_same<decltype(ix.text()), const Sym *>::value, "the query has the text's symbol type");
    if (!q_off) ndocs = 1;
    const ScoreLayout L = score_layout(m, ndocs);
    if (m > 0 && (!dQ || !dWork || work_bytes < (int64_t)L.bytes || (((uintptr_t)dWork) & 255u) || (((uintptr_t)dQ) & (sizeof(Sym) - 1))))
        return SA_AMD_EINVAL;
    Stats ss;
    memset(&ss, 0, sizeof(ss));
    const int cap = g_score_cap < 0 ? SCORE_CAP_DEFAULT : g_score_cap;
    int ge = cap < SCORE_STAGE_MAX ? cap : SCORE_STAGE_MAX;
    if (ge > max_len) ge = max_len;
    ss.positions = m;
    ss.documents = ndocs;
    ss.group_cap = ge;
    last = ss;
    if (m == 0) return SA_AMD_OK;
    route_tuning();                                             // (the posted read-backs' switch; nothing else of the tuning is used here)
    const int rb0 = g_readbacks;
    char *base = (char *)dWork;
    unsigned long long *ctl = (unsigned long long *)(base + L.ctl);
    int64_t *dOff = q_off ? (int64_t *)(base + L.off) : nullptr;
    uint32_t *list = (uint32_t *)(base + L.list), *llo = (uint32_t *)(base + L.lo), *lhi = (uint32_t *)(base + L.hi);
    HIP_TRY(hipMemsetAsync(ctl, 0, 256, st));
    if (q_off) HIP_TRY(hipMemcpyAsync(dOff, q_off, ((size_t)ndocs + 1) * 8, hipMemcpyHostToDevice, st));

    // ---- pass 1: the group path ----
    PROF(KC_MISC, m, st, hipLaunchKernelGGL((k_score_tile<SCORE_G, Sym>), dim3((unsigned)ceil_div(m, SCORE_TILE)), dim3(SCORE_THREADS),
                                            (size_t)score_stage_words<Sym>(ge) * 4, st, ix.text(), ix.sa(), (int64_t)ix.n, ix.bkt(), dQ, m, (const int64_t *)dOff,
                                            ndocs, (uint32_t)min_count, (int64_t)max_len, ge, out, list, llo, lhi, ctl));
    unsigned long long cw[SC_W_COUNT];
    { const int rcw = read_words(cw, ctl, sizeof(cw), st); if (rcw) return rcw; }
    const int64_t longs = (int64_t)(uint32_t)cw[SC_W_LONG];
    if (longs > m) return SA_AMD_EINTERNAL;

    // ---- pass 2: one wave per listed position ----
    if (longs > 0) {
        PROF(KC_MISC, longs, st, hipLaunchKernelGGL(k_score_long<Sym>, dim3((unsigned)ceil_div(longs * WAVE, SCORE_THREADS)), dim3(SCORE_THREADS), 0, st, ix.text(),
                                                    ix.sa(), (int64_t)ix.n, ix.bkt(), ix.pair(), esa_log_p(ix.n), dQ, m, (const int64_t *)dOff, ndocs,
                                                    (uint32_t)min_count, (int64_t)max_len, ge, (const uint32_t *)list, (const uint32_t *)llo,
                                                    (const uint32_t *)lhi, longs, out, ctl));
        const int rcw = read_words(cw, ctl, sizeof(cw), st);
        if (rcw) return rcw;
    }
    HIP_TRY(hipStreamSynchronize(st));
    g_prof.resolve();
    ss.long_positions = longs;
    ss.group_searches = (int64_t)cw[SC_W_GROUP_SEARCHES];
    ss.long_searches = (int64_t)cw[SC_W_LONG_SEARCHES];
    ss.next_lookups = (int64_t)cw[SC_W_LOOKUPS];
    ss.*compared = (int64_t)cw[SC_W_BYTES];
    ss.zero_positions = (int64_t)cw[SC_W_ZERO];
    ss.readbacks = g_readbacks - rb0;
    last = ss;
    return SA_AMD_OK;
}

// host buffers: the query goes up (sizeof(Sym) m bytes), the outputs asked for come back (4 m bytes each, AT_END m).  One pooled
// block.
template <typename Index, typename Sym, typename Stats>
static int score_host(const Index &ix, const Sym *Q, int64_t m, const int64_t *q_off, int64_t ndocs, int32_t min_count, int32_t max_len,
                      uint32_t *S, uint32_t *LO, uint32_t *HI, uint8_t *AT_END, uint32_t *NLO, uint32_t *NHI, Stats &last, int64_t Stats::*compared)
{
    const size_t wb = score_layout(m, q_off ? ndocs : 1).bytes, eb = align_up((size_t)m + 16, 256), qb = align_up(sizeof(Sym) * (size_t)m + 16, 256),
                 ab = align_up(((size_t)m + 1) * 4, 256);
    uint32_t *const host4[5] = { S, LO, HI, NLO, NHI };
    uint32_t *dev4[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    size_t outs = AT_END ? eb : 0;
    for (int k = 0; k < 5; ++k) outs += host4[k] ? ab : 0;
    PooledScope sc(ix.device, true);
    sc.acquire(wb + qb + outs);
    void *dW = sc.take(wb);
    Sym *dQ = (Sym *)sc.take(qb);
    for (int k = 0; k < 5; ++k)
        if (host4[k]) dev4[k] = (uint32_t *)sc.take(ab);
    uint8_t *dEnd = AT_END ? (uint8_t *)sc.take(eb) : nullptr;
    if (sc.rc == SA_AMD_OK && m > 0) sc.rc = hip_status(hipMemcpyAsync(dQ, Q, sizeof(Sym) * (size_t)m, hipMemcpyHostToDevice, sc.st));
    if (sc.rc == SA_AMD_OK) {
        ScoreOut out;
        out.S = dev4[0]; out.LO = dev4[1]; out.HI = dev4[2]; out.AT_END = dEnd; out.NLO = dev4[3]; out.NHI = dev4[4];
        sc.rc = score_device(ix, dQ, m, q_off, ndocs, min_count, max_len, out, dW, (int64_t)wb, sc.st, last, compared);
    }
    for (int k = 0; k < 5; ++k)
        if (m > 0 && host4[k]) sc.down(host4[k], dev4[k], (size_t)m * 4);
    if (m > 0 && AT_END) sc.down(AT_END, dEnd, (size_t)m);
    return sc.finish();
}

}  // namespace sa
