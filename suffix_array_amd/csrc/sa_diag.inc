// sa_diag.inc -- entry points that exist ONLY in libsuffix_array_amd_diag.so (-DSA_AMD_DIAG; declared in
// csrc/sa_diag.h, not in include/): phase-stamp read-out of the diagnostic kernels and hooks that run one primitive
// (radix sort, key packing) on host buffers so that tests/ can localise a failing kernel.  Included inside the
// extern "C" block of sa_api.hip.

SA_EXPORT int32_t sa_amd_debug_phase_cycles(uint64_t *out, int32_t count)
{
    unsigned long long h[16] = { 0 };
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(sa::g_phase_cycles), sizeof(h)) != hipSuccess) return SA_AMD_EHIP;
    for (int i = 0; i < count && i < 16; ++i) out[i] = h[i];
    unsigned long long z[16] = { 0 };
    (void)hipMemcpyToSymbol(HIP_SYMBOL(sa::g_phase_cycles), z, sizeof(z));
    return 16;
}

SA_EXPORT int32_t sa_amd_debug_group_sort_stamps(int32_t on)
{
    const int v = on ? 1 : 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(sa::g_gs_stamp_on), &v, sizeof(v)) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

SA_EXPORT int32_t sa_amd_debug_rr_count_stamps(int32_t on)
{
    const int v = on ? 1 : 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(sa::g_rr_stamp_on), &v, sizeof(v)) == hipSuccess ? SA_AMD_OK : SA_AMD_EHIP;
}

SA_EXPORT int32_t sa_amd_debug_rerank_routes(int32_t flags)
{
    return sa::g_rerank_routes.exchange(flags & 3);
}

SA_EXPORT int32_t sa_amd_debug_doc_tf_bounds(int32_t mode)
{
    return sa::g_doc_tf_plain_bounds.exchange(mode ? 1 : 0);
}

SA_EXPORT int32_t sa_amd_debug_fill_blocks(int32_t pattern)
{
    return sa::g_fill_pattern.exchange(pattern < 0 || pattern > sa::FILL_RANDOM ? sa::FILL_OFF : pattern);
}

SA_EXPORT int32_t sa_amd_debug_refuse_alloc(int32_t nth)
{
    sa::RefuseSwitch &r = sa::g_refuse;
    const int32_t made = r.count;
    r.nth = nth < -1 ? -1 : nth;
    r.count = 0;
    r.fired = false;
    return made;
}

SA_EXPORT int32_t sa_amd_debug_refuse_fired(void) { return sa::g_refuse.fired ? 1 : 0; }

SA_EXPORT int32_t sa_amd_debug_refuse_kinds(uint8_t *kinds, int32_t capacity)
{
    const sa::RefuseSwitch &r = sa::g_refuse;
    const int have = r.count < sa::DIAG_KINDS_MAX ? r.count : sa::DIAG_KINDS_MAX;
    for (int i = 0; kinds && i < have && i < capacity; ++i) kinds[i] = r.kinds[i];
    return r.count;
}

SA_EXPORT int32_t sa_amd_debug_live_allocations(int64_t *device, int64_t *pinned)
{
    if (!device || !pinned) return SA_AMD_EINVAL;
    *device = sa::g_live_device.load(std::memory_order_relaxed);
    *pinned = sa::g_live_pinned.load(std::memory_order_relaxed);
    return SA_AMD_OK;
}

SA_EXPORT int32_t sa_amd_debug_dsub_plain_atomics(int32_t mode)
{
    return sa::g_dsub_plain_atomics.exchange(mode ? 1 : 0);
}

SA_EXPORT int32_t sa_amd_debug_head_flags(int32_t mode)
{
    return sa::g_head_flags_mode.exchange(mode < 0 ? 0 : (mode > 2 ? 2 : mode));
}

SA_EXPORT int32_t sa_amd_debug_round_flags(int32_t mode)
{
    return sa::g_round_flags_mode.exchange(mode < 0 ? 0 : (mode > 2 ? 2 : mode));
}

SA_EXPORT int32_t sa_amd_debug_sort_variant_count(void) { return sa::N_SORT_VARIANTS; }
SA_EXPORT const char *sa_amd_debug_sort_variant_name(int32_t i)
{
    return (i >= 0 && i < sa::N_SORT_VARIANTS) ? sa::sort_variants[i].name : "";
}

SA_EXPORT int32_t sa_amd_test_sort_pairs(uint64_t *keys, uint32_t *vals, int64_t count, int32_t begin_bit, int32_t end_bit)
{
    using namespace sa;
    if (count < 0 || (count > 0 && (!keys || !vals)) || begin_bit < 0 || end_bit > 64) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    if (count == 0) return SA_AMD_OK;
    const Tuning tn = env_tuning();
    const size_t N = (size_t)count;
    DevBuf dk, dv, dsp;
    int32_t rc;
    if ((rc = dk.alloc(N * 8 * 2))) return rc;
    if ((rc = dv.alloc(N * 4 * 2))) return rc;
    if ((rc = dsp.alloc(SortScratch::SPINE_BYTES))) return rc;
    uint64_t *k = dk.as<uint64_t>(); uint32_t *v = dv.as<uint32_t>();
    HIP_TRY(hipMemcpy(k, keys, N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v, vals, N * 4, hipMemcpyHostToDevice));
    SortResult<uint64_t> sr;
    DevBuf dst;
    if ((rc = dst.alloc(256 + SortScratch::granule_bytes(count)))) return rc;
    HIP_TRY(hipMemset(dst.p, 0, 256));
    const SortScratch ss = SortScratch::make(dsp.p, dst.as<char>() + 256, dst.as<uint32_t>());      // (the error words in front of the granules)
    rc = sort_pairs(SortJob<uint64_t>{ k, v, k + N, v + N, count, begin_bit, end_bit }, ss, nullptr, tn, &sr);
    if (rc != SA_AMD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(keys, sr.keys, N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals, sr.vals, N * 4, hipMemcpyDeviceToHost));
    { uint32_t e = 0; HIP_TRY(hipMemcpy(&e, ss.err, 4, hipMemcpyDeviceToHost)); if (e) return SA_AMD_EINTERNAL; }
    return SA_AMD_OK;
}

// The same sort with the flags variant of the last pass (k_onesweep<..., HEAD_FLAGS>; single-pass engine only): vals = the sorted
// order, flags_out[count] = the group-start flags, keys_out[count] = that pass's key buffer, filled with 0xA5 bytes in front of it
// (only the keys at the ends of the tiles' digit runs are stored).  `keys` is not written.  count == 1: no pass runs, flag 1.
SA_EXPORT int32_t sa_amd_test_sort_pairs_flags(const uint64_t *keys, uint32_t *vals, int64_t count, int32_t begin_bit, int32_t end_bit,
                                               uint8_t *flags_out, uint64_t *keys_out)
{
    using namespace sa;
    if (count <= 0 || !keys || !vals || !flags_out || !keys_out || begin_bit < 0 || end_bit > 64 || end_bit <= begin_bit) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    const Tuning tn = env_tuning();
    const size_t N = (size_t)count;
    memset(keys_out, 0xA5, N * 8);
    if (count == 1) { flags_out[0] = OS_HF_START; return SA_AMD_OK; }
    DevBuf dk, dv, dsp, dst, df;
    int32_t rc;
    if ((rc = dk.alloc(N * 8 * 2))) return rc;
    if ((rc = dv.alloc(N * 4 * 3))) return rc;
    if ((rc = df.alloc(N))) return rc;
    if ((rc = dsp.alloc(SortScratch::SPINE_BYTES))) return rc;
    if ((rc = dst.alloc(256 + SortScratch::granule_bytes(count)))) return rc;
    uint64_t *k = dk.as<uint64_t>(); uint32_t *v = dv.as<uint32_t>();
    HIP_TRY(hipMemcpy(k, keys, N * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v, vals, N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(df.p, 0xff, N));
    HIP_TRY(hipMemset(dst.p, 0, 256));
    const SortScratch ss = SortScratch::make(dsp.p, dst.as<char>() + 256, dst.as<uint32_t>());      // (the error words in front of the granules)
    if (!onesweep_on(ss, tn)) return SA_AMD_EINVAL;      // (the three-kernel engine has no flags variant)
    SortJob<uint64_t> job{ k, v, k + N, v + N, count, begin_bit, end_bit };
    job.final_vals = v + 2 * N;
    job.head_flags = df.as<uint8_t>(); job.poison_keys = true;
    SortResult<uint64_t> sr;
    rc = sort_pairs(job, ss, nullptr, tn, &sr);
    if (rc != SA_AMD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (sr.vals != v + 2 * N) return SA_AMD_EINTERNAL;
    HIP_TRY(hipMemcpy(keys_out, sr.keys, N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals, sr.vals, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags_out, df.p, N, hipMemcpyDeviceToHost));
    { uint32_t e = 0; HIP_TRY(hipMemcpy(&e, ss.err, 4, hipMemcpyDeviceToHost)); if (e) return SA_AMD_EINTERNAL; }
    return SA_AMD_OK;
}

// the sample sort of the 64-bit stage (kernels/sample_sort.hpp) on host arrays: keys[0 .. count) in, the keys in order and the
// index each one came from out; *done = 0: a bucket that is no equality bucket did not fit a workgroup (outputs undefined)
SA_EXPORT int32_t sa_amd_test_sample_sort64(uint64_t *keys, uint32_t *vals, int64_t count, int32_t key_bits, int32_t *done)
{
    using namespace sa;
    if (count <= 0 || !keys || !vals || !done || key_bits < 1 || key_bits > 64) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    const Tuning tn = env_tuning();
    const size_t N = (size_t)count;
    DevBuf dk, dv, dsp, dst, dbig, dsmall;
    int32_t rc;
    if ((rc = dk.alloc((N + 64) * 8 * 3))) return rc;
    if ((rc = dv.alloc(N * 4 * 5))) return rc;
    if ((rc = dsp.alloc(SortScratch::SPINE_BYTES))) return rc;
    if ((rc = dst.alloc(256 + SortScratch::granule_bytes(count)))) return rc;
    if ((rc = dbig.alloc(((size_t)ceil_div(count, SS_TILE) + SS_WAYS) * SS_IDS2 * 4))) return rc;
    if ((rc = dsmall.alloc((size_t)8 << 20))) return rc;
    HIP_TRY(hipMemset(dst.p, 0, 256));
    uint64_t *k = dk.as<uint64_t>();
    uint32_t *v = dv.as<uint32_t>();
    HIP_TRY(hipMemcpy(k, keys, N * 8, hipMemcpyHostToDevice));
    const SortScratch ss = SortScratch::make(dsp.p, dst.as<char>() + 256, dst.as<uint32_t>());      // (the error words in front of the granules)
    sa_amd_stats local;
    memset(&local, 0, sizeof(local));
    bool ok = false;
    uint32_t *words = dsmall.as<uint32_t>() + ((size_t)6 << 18);           // (behind the 6 MiB the sort's small arrays may take)
    rc = sample_sort64(k, k + (N + 64), k + 2 * (N + 64), v, v + N, v + 2 * N, v + 3 * N, dbig.as<uint32_t>(), dsmall.as<uint32_t>(), words,
                       v + 4 * N, count, key_bits, ss, nullptr, &local, tn, &ok, false);
    if (rc != SA_AMD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *done = ok ? 1 : 0;
    if (ok) {
        HIP_TRY(hipMemcpy(keys, k + (N + 64), N * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(vals, v + 4 * N, N * 4, hipMemcpyDeviceToHost));
    }
    { uint32_t e = 0; HIP_TRY(hipMemcpy(&e, ss.err, 4, hipMemcpyDeviceToHost)); if (e) return SA_AMD_EINTERNAL; }
    return SA_AMD_OK;
}

SA_EXPORT int32_t sa_amd_test_sort_pairs32(uint32_t *keys, uint32_t *vals, int64_t count, int32_t begin_bit, int32_t end_bit)
{
    using namespace sa;
    if (count < 0 || (count > 0 && (!keys || !vals)) || begin_bit < 0 || end_bit > 32) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    if (count == 0) return SA_AMD_OK;
    const Tuning tn = env_tuning();
    const size_t N = ((size_t)count + 3) & ~(size_t)3;
    DevBuf dk, dv, dsp;
    int32_t rc;
    if ((rc = dk.alloc(N * 4 * 2))) return rc;
    if ((rc = dv.alloc(N * 4 * 2))) return rc;
    if ((rc = dsp.alloc(SortScratch::SPINE_BYTES))) return rc;
    uint32_t *k = dk.as<uint32_t>(), *v = dv.as<uint32_t>();
    HIP_TRY(hipMemcpy(k, keys, (size_t)count * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v, vals, (size_t)count * 4, hipMemcpyHostToDevice));
    SortResult<uint32_t> sr;
    DevBuf dst;
    if ((rc = dst.alloc(256 + SortScratch::granule_bytes(count)))) return rc;
    HIP_TRY(hipMemset(dst.p, 0, 256));
    const SortScratch ss = SortScratch::make(dsp.p, dst.as<char>() + 256, dst.as<uint32_t>());      // (the error words in front of the granules)
    rc = sort_pairs32(SortJob<uint32_t>{ k, v, k + N, v + N, count, begin_bit, end_bit }, ss, nullptr, tn, &sr);
    if (rc != SA_AMD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(keys, sr.keys, (size_t)count * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals, sr.vals, (size_t)count * 4, hipMemcpyDeviceToHost));
    { uint32_t e = 0; HIP_TRY(hipMemcpy(&e, ss.err, 4, hipMemcpyDeviceToHost)); if (e) return SA_AMD_EINTERNAL; }
    return SA_AMD_OK;
}

__global__ void k_test_count_digit(const uint32_t *keys, int64_t n, int shift, uint32_t dmask, uint32_t *counts, int64_t chunk_elems, int G)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&counts[(int64_t)((keys[i] >> shift) & dmask) * G + i / chunk_elems], 1u);
}

// two global passes over the top 16 (or 18: nine-bit digits) key bits + the in-LDS bucket sort of the rest (kernels/bucket_sort.hpp), host buffers;
// *largest = the largest bucket; returns 1 when it is larger than every workgroup shape holds (buffers untouched)
SA_EXPORT int32_t sa_amd_test_bucket_sort32(uint32_t *keys, uint32_t *vals, int64_t count, int32_t top_bits, uint32_t *largest)
{
    using namespace sa;
    if (count < 0 || (count > 0 && (!keys || !vals)) || !largest || (top_bits != 16 && top_bits != 18)) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    *largest = 0;
    if (count == 0) return SA_AMD_OK;
    const Tuning tn = env_tuning();
    const size_t N = ((size_t)count + 3) & ~(size_t)3;
    DevBuf dk, dv, dsp, dst, dbs;
    int32_t rc;
    if ((rc = dk.alloc(N * 4 * 2))) return rc;
    if ((rc = dv.alloc(N * 4 * 3))) return rc;
    if ((rc = dsp.alloc(SortScratch::SPINE_BYTES))) return rc;
    if ((rc = dst.alloc(256 + SortScratch::granule_bytes(count)))) return rc;
    if ((rc = dbs.alloc(((size_t)BK_BUCKETS_MAX + 1) * 4))) return rc;
    uint32_t *k = dk.as<uint32_t>(), *v = dv.as<uint32_t>();
    HIP_TRY(hipMemcpy(k, keys, (size_t)count * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v, vals, (size_t)count * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dst.p, 0, 256));
    const SortScratch ss = SortScratch::make(dsp.p, dst.as<char>() + 256, dst.as<uint32_t>());      // (the error words in front of the granules)
    SortResult<uint32_t> sr;
    const int rbits = top_bits == 18 ? 9 : RADIX_BITS;
    bool counted = false;
    if (rbits == 9) {
        // (a nine-bit first digit is counted by the producer of the keys: here, by a small counting kernel over the host's keys)
        const FirstCounts fc = sort_first_counts(ss, tn, count, true);
        HIP_TRY(hipMemset(fc.zero_ptr, 0, fc.zero_bytes));
        hipLaunchKernelGGL(k_test_count_digit, dim3(256), dim3(256), 0, nullptr, (const uint32_t *)k, count, 32 - top_bits, 511u, fc.counts, fc.chunk_elems, fc.G);
        HIP_TRY(hipGetLastError());
        counted = true;
    }
    SortJob<uint32_t> job{ k, v, k + N, v + N, count, 32 - top_bits, 32 };
    job.first_counted = counted; job.rbits = rbits;
    rc = sort_pairs32(job, ss, nullptr, tn, &sr);
    if (rc != SA_AMD_OK) return rc;
    uint32_t *kout = sr.keys == k ? k + N : k, *vout = v + 2 * N;
    bool done = false;
    rc = bucket_sort32(sr.keys, sr.vals, kout, vout, count, top_bits, dbs.as<uint32_t>(), ss.err + 2, nullptr, tn, &done, largest);
    if (rc != SA_AMD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    { uint32_t e[4] = { 0, 0, 0, 0 }; HIP_TRY(hipMemcpy(e, ss.err, 16, hipMemcpyDeviceToHost)); if (e[0] || e[3]) return SA_AMD_EINTERNAL; }
    if (!done) return 1;
    HIP_TRY(hipMemcpy(keys, kout, (size_t)count * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals, vout, (size_t)count * 4, hipMemcpyDeviceToHost));
    return SA_AMD_OK;
}

SA_EXPORT int32_t sa_amd_test_build_keys(const uint8_t *T, int32_t n, uint64_t *keys, int32_t *bits, int32_t *k)
{
    using namespace sa;
    if (n <= 0 || !T || !keys) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    DevBuf dT, dk, dv, dh;
    int32_t rc;
    if ((rc = dT.alloc((size_t)n))) return rc;
    if ((rc = dk.alloc((size_t)n * 8))) return rc;
    if ((rc = dv.alloc((size_t)n * 4))) return rc;
    if ((rc = dh.alloc(1024))) return rc;
    HIP_TRY(hipMemcpy(dT.p, T, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dh.p, 0, 1024));
    int64_t blocks = ceil_div(ceil_div((int64_t)n, 16), BH_THREADS);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_byte_hist, dim3((unsigned)blocks), dim3(BH_THREADS), 0, nullptr, dT.as<const uint8_t>(), (int64_t)n, dh.as<uint32_t>());
    uint32_t hist[256];
    HIP_TRY(hipMemcpy(hist, dh.p, 1024, hipMemcpyDeviceToHost));
    KeyParams P; int sigma;
    make_key_params(hist, &P, &sigma);
    hipLaunchKernelGGL((k_build_keys<false>), dim3((unsigned)ceil_div(ceil_div((int64_t)n, KB_TILE), KB_TPW)), dim3(KB_THREADS), 0, nullptr, dT.as<const uint8_t>(),
                       (int64_t)n, P, dk.as<uint64_t>(), dv.as<uint32_t>(), (uint32_t *)nullptr, 0, (uint8_t *)nullptr,
                       (uint32_t *)nullptr, (int64_t)KB_TILE, 1, 0u);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(keys, dk.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (bits) *bits = P.bits;
    if (k) *k = P.k;
    return SA_AMD_OK;
}

// one exact level-0 L-type induce sweep by a single wavefront (kernels/induce_proto.hpp); host buffers:
// SA (n + 1 slots, LMS suffixes placed, the rest 0xffffffff) is updated in place; returns the kernel time in *ms
SA_EXPORT int32_t sa_amd_proto_induce_l(const uint8_t *T, const uint8_t *typeL, uint32_t *SA, int32_t n, const uint32_t *head,
                                        double *ms, uint64_t *counters)
{
    using namespace sa;
    if (n <= 0 || !T || !typeL || !SA || !head || !ms || !counters) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    const size_t N = (size_t)n;
    DevBuf dT, dL, dS, dH, dC;
    int32_t rc;
    if ((rc = dT.alloc(N))) return rc;
    if ((rc = dL.alloc(N / 8 + 8))) return rc;
    if ((rc = dS.alloc((N + 1) * 4))) return rc;
    if ((rc = dH.alloc(1024))) return rc;
    if ((rc = dC.alloc(16))) return rc;
    HIP_TRY(hipMemcpy(dT.p, T, N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dL.p, typeL, N / 8 + 1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dS.p, SA, (N + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dH.p, head, 1024, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dC.p, 0, 16));
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, nullptr));
    hipLaunchKernelGGL(k_induce_l_sweep, dim3(1), dim3(64), 0, nullptr, dT.as<const uint8_t>(), dL.as<const uint8_t>(), dS.as<uint32_t>(),
                       (int64_t)n, dH.as<const uint32_t>(), dC.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b, nullptr));
    HIP_TRY(hipEventSynchronize(b));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    *ms = t;
    HIP_TRY(hipMemcpy(SA, dS.p, (N + 1) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counters, dC.p, 16, hipMemcpyDeviceToHost));
    return SA_AMD_OK;
}

// stage 1 of the Lempel-Ziv factorisation (kernels/lz.hpp) alone, on a device array of n distinct uint32 values: the nearest
// slot to the left / right that holds a smaller value to dPsv / dNsv (n entries each, device; 0xffffffff: none).  counters
// (host, four words): slots unresolved inside their tile, words loaded from the levels, the most for one side of one slot, levels.
SA_EXPORT int32_t sa_amd_test_lz_nsv(const uint32_t *dA, int64_t n, uint32_t *dPsv, uint32_t *dNsv, int64_t *counters)
{
    using namespace sa;
    if (n <= 0 || n > 0x7fffffffLL || !dA || !dPsv || !dNsv || !counters) return SA_AMD_EINVAL;
    if (sa::device_count() <= 0) return SA_AMD_ENODEVICE;
    DevBuf dl, dc;
    int32_t rc;
    if ((rc = dl.alloc(((size_t)n / 31 + 64) * 4))) return rc;
    if ((rc = dc.alloc(256))) return rc;
    HIP_TRY(hipMemset(dc.p, 0, 256));
    rc = lz_nsv(dA, n, dPsv, dNsv, dl.as<uint32_t>(), nullptr, nullptr, dc.as<unsigned long long>(), nullptr);
    if (rc != SA_AMD_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long cw[LZ_C_WORDS];
    HIP_TRY(hipMemcpy(cw, dc.p, sizeof(cw), hipMemcpyDeviceToHost));
    counters[0] = (int64_t)cw[LZ_C_UNRES];
    counters[1] = (int64_t)cw[LZ_C_HSTEPS];
    counters[2] = (int64_t)cw[LZ_C_HMAX];
    counters[3] = lz_levels(n, nullptr).top;
    return SA_AMD_OK;
}
