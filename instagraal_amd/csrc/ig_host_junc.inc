/* ig_host_junc.inc -- part of ig_hip.hip (one translation unit; included there in order): the junction support profile of the
 * current genome (ig_kernels_junc.cuh; the rule: instagraal_amd/junction_profile.py). */

/* the three arrays of JuncBuf.diff / JuncBuf.prof, M + 1 words each */
#define JUNC_ARR_OBS 0
#define JUNC_ARR_PAIRS 1
#define JUNC_ARR_EXP 2

/* the form of the observed pass ig_junction_profile runs: 1 equal + ends combined inside the wave, 0 one atomic per end (the
 * yardstick).  The combined form ships only once its median is measured not above the yardstick's at cfg3 and cfg3_late
 * (tools/junction_profile_bench.py -> profiles/r09_junction_profile.json, DESIGN.md 4.12): not shown yet */
#define JUNC_SHIP_COMBINE 0

static void free_junc_buffers(ig_ctx* c)
{
    hipFree(c->junc.diff);
    hipFree(c->junc.prof);
    hipFree(c->junc.tot);
    hipFree(c->junc.sc);
    c->junc = JuncBuf{};
}

/* Argument checks, the genome view (its guards, the records by position, ds and meta), the buffers, the number of internal
 * junctions.  T: placed sub-fragments. */
static int junc_prepare(ig_ctx* c, const char* who, int window, bool want_model, int* T_out)
{
    if (check_window(who, window)) return -1;
    if (genome_positions(c, who, GENOME_RECORDS | GENOME_SORTED, T_out)) return -1;
    if (want_model && !c->have_params) return fail("%s: set parameters first", who);
    JuncBuf& j = c->junc;
    const int M = c->M;
    if (j.M != M) {
        free_junc_buffers(c);
        DALLOC(j.diff, 3 * ((size_t)M + 1));
        DALLOC(j.prof, 3 * ((size_t)M + 1));
        DALLOC(j.tot, 3 * (size_t)scan_chunks(M + 1));
        DALLOC(j.sc, (size_t)JUNC_NS);
        j.M = M;
    }
    const int T = *T_out;
    HIPCK(hipMemsetAsync(j.sc, 0, JUNC_NS * sizeof(unsigned long long), c->stream));
    if (T > 0) hipLaunchKernelGGL(k_junc_count, dim3((T + JUNC_THREADS - 1) / JUNC_THREADS), dim3(JUNC_THREADS), 0, c->stream, c->genome.meta, T, j.sc + JUNC_INTERNAL);
    return 0;
}

/* zero + the observed pass on the library's stream */
static int junc_enqueue_observed(ig_ctx* c, int T, int window, bool combine)
{
    JuncBuf& j = c->junc;
    unsigned long long* diff = j.diff + (size_t)JUNC_ARR_OBS * ((size_t)j.M + 1);
    HIPCK(hipMemsetAsync(diff, 0, ((size_t)T + 1) * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(j.sc, 0, JUNC_N_OBS * sizeof(unsigned long long), c->stream));
    if (c->Z == 0) return 0;
    const int blocks = (int)std::min<long long>((c->Z + JUNC_THREADS - 1) / JUNC_THREADS, 4096);
    const bool narrow = c->max_count < (1 << 25); /* 64 counts fit an int */
    if (combine && narrow)
        hipLaunchKernelGGL((k_junc_observed<true, int>), dim3(blocks), dim3(JUNC_THREADS), 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, window, diff, j.sc, c->rank, c->world);
    else if (combine)
        hipLaunchKernelGGL((k_junc_observed<true, long long>), dim3(blocks), dim3(JUNC_THREADS), 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, window, diff, j.sc, c->rank, c->world);
    else
        hipLaunchKernelGGL((k_junc_observed<false, int>), dim3(blocks), dim3(JUNC_THREADS), 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, window, diff, j.sc, c->rank, c->world);
    return 0;
}

/* the model pass: every word of both arrays is written by the position that owns it */
static int junc_enqueue_model(ig_ctx* c, int T, int window)
{
    JuncBuf& j = c->junc;
    const size_t stride = (size_t)j.M + 1;
    HIPCK(hipMemsetAsync(j.sc + JUNC_DEV_MAXQ, 0, sizeof(unsigned long long), c->stream));
    if (T == 0) return 0;
    if (window > JUNC_WAVE_WINDOW)
        hipLaunchKernelGGL((k_junc_model<64>), dim3((unsigned)(((long long)T * 64 + JUNC_THREADS - 1) / JUNC_THREADS)), dim3(JUNC_THREADS), 0, c->stream, c->genome.ds, c->genome.meta, T,
                           window, c->glob, j.diff + JUNC_ARR_PAIRS * stride, j.diff + JUNC_ARR_EXP * stride, j.sc + JUNC_DEV_MAXQ);
    else
        hipLaunchKernelGGL((k_junc_model<1>), dim3((T + JUNC_THREADS - 1) / JUNC_THREADS), dim3(JUNC_THREADS), 0, c->stream, c->genome.ds, c->genome.meta, T, window, c->glob,
                           j.diff + JUNC_ARR_PAIRS * stride, j.diff + JUNC_ARR_EXP * stride, j.sc + JUNC_DEV_MAXQ);
    return 0;
}

/* the prefix sums of the first n_arrays difference arrays: diff -> prof (diff stays as it is: the scan can be repeated) */
static int junc_enqueue_scan(ig_ctx* c, int T, int n_arrays)
{
    JuncBuf& j = c->junc;
    scan64_enqueue(c, j.diff, j.prof, (long long)j.M + 1, T + 1, n_arrays, j.tot);
    return 0;
}

extern "C" int ig_junction_profile(ig_ctx* c, int32_t window, int64_t* observed, int64_t* pairs, int64_t* expected_q, int64_t capacity,
                                   int32_t* n_placed, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!observed || !n_placed || !scalars) return fail("ig_junction_profile: NULL output");
    if ((pairs == nullptr) != (expected_q == nullptr)) return fail("ig_junction_profile: NULL output (pairs and expected_q go together)");
    const bool model = pairs != nullptr;
    int T = 0;
    if (junc_prepare(c, "ig_junction_profile", window, model, &T)) return -1;
    *n_placed = T;
    if (capacity < T) return fail("ig_junction_profile: the profile has %d entries, the caller's capacity is %lld", T, (long long)capacity);
    if (junc_enqueue_observed(c, T, window, JUNC_SHIP_COMBINE != 0)) return -1;
    if (model) {
        if (junc_enqueue_model(c, T, window)) return -1;
        if (check_model_sum(c, "ig_junction_profile", c->junc.sc + JUNC_DEV_MAXQ, window)) return -1;
    }
    if (junc_enqueue_scan(c, T, model ? 3 : 1)) return -1;
    JuncBuf& j = c->junc;
    const size_t stride = (size_t)j.M + 1;
    long long sc[JUNC_NS];
    HIPCK(hipMemcpyAsync(sc, j.sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    if (T > 0) {
        HIPCK(hipMemcpyAsync(observed, j.prof + JUNC_ARR_OBS * stride, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        if (model) {
            HIPCK(hipMemcpyAsync(pairs, j.prof + JUNC_ARR_PAIRS * stride, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCK(hipMemcpyAsync(expected_q, j.prof + JUNC_ARR_EXP * stride, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCK(hipStreamSynchronize(c->stream));
    long long spanned = 0;
    for (int r = 0; r < T; r++) spanned += observed[r];
    for (int k = 0; k < JUNC_NS; k++) scalars[k] = k <= JUNC_INTERNAL ? sc[k] : 0;
    scalars[JUNC_SPANNED] = spanned;
    return 0;
}

extern "C" int ig_debug_junction_profile_time(ig_ctx* c, int32_t window, int32_t combine, int32_t n, float* ms_observed_n, float* ms_model_n,
                                              float* ms_scan_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_observed_n) return fail("ig_debug_junction_profile_time: bad arguments");
    int T = 0;
    if (junc_prepare(c, "ig_debug_junction_profile_time", window, ms_model_n != nullptr, &T)) return -1;
    const char* who = "ig_debug_junction_profile_time";
    if (time_repeats(c, who, n, ms_observed_n, [&] { return junc_enqueue_observed(c, T, window, combine != 0); })) return -1;
    if (ms_model_n && time_repeats(c, who, n, ms_model_n, [&] { return junc_enqueue_model(c, T, window); })) return -1;
    /* (the scan runs once where nobody asked for its time: the checksum needs it) */
    if (time_repeats(c, who, ms_scan_n ? n : 1, ms_scan_n, [&] { return junc_enqueue_scan(c, T, ms_model_n ? 3 : 1); })) return -1;
    if (checksum) { /* of the last observed pass behind the scan, every word weighted by its place: both forms of the kernel must agree on it */
        std::vector<long long> h((size_t)T + JUNC_N_OBS, 0);
        if (T > 0) HIPCK(hipMemcpy(h.data(), c->junc.prof, (size_t)T * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(h.data() + T, c->junc.sc, JUNC_N_OBS * sizeof(long long), hipMemcpyDeviceToHost));
        *checksum = (long long)weighted_checksum(h.data(), h.size());
    }
    return 0;
}
