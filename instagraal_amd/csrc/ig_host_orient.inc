/* ig_host_orient.inc -- part of ig_hip.hip (one translation unit; included there in order): orientation support, which segments of
 * the current genome the contacts would reverse (ig_kernels_orient.cuh; the rule: instagraal_amd/orientation_support.py). */

/* the form of the observed pass ig_orientation_support runs: 1 equal row ends combined inside the wave, 0 one atomic per counted end
 * (the yardstick).  The combined form ships only once its median is measured not above the yardstick's at cfg3 and cfg3_late
 * (tools/orientation_support_bench.py -> profiles/r14_orientation_support.json, DESIGN.md 4.18): not timed yet */
#define ORIENT_SHIP_COMBINE 0

/* the passes and forms of ig_debug_orientation_support_time */
#define ORIENT_PASS_OBSERVED 0 /* form 0: one atomic per counted end, 1: combined inside the wave */
#define ORIENT_PASS_MODEL 1    /* form 0: as shipped (ORIENT_WAVE_PAIRS), 1: a wave per segment, 2: a workgroup per judged segment */

static void free_orient_buffers(ig_ctx* c)
{
    OrientBuf& o = c->orient;
    hipFree(o.seg);
    hipFree(o.first);
    hipFree(o.last);
    hipFree(o.geo);
    hipFree(o.bnd);
    hipFree(o.large);
    hipFree(o.obs);
    hipFree(o.expq);
    hipFree(o.sc);
    hipFree(o.ctl);
    o = OrientBuf{};
}

/* Argument checks, the genome view (its guards, the records by position, ds and meta), the buffers, the list on the device: checked,
 * its geometry, seg[] painted.  T: placed sub-fragments; n_large: segments listed for the workgroup form of the model pass under
 * wave_pairs.  Waits for the stream (the error word). */
static int orient_prepare(ig_ctx* c, const char* who, int window, bool want_model, int n_seg, const int32_t* first, const int32_t* last, long long wave_pairs,
                          int* T_out, int* n_large)
{
    if (check_window(who, window)) return -1;
    if (n_seg < 0) return fail("%s: segment list of %d entries", who, n_seg);
    if (n_seg > 0 && (!first || !last)) return fail("%s: NULL segment list", who);
    if (genome_positions(c, who, GENOME_RECORDS | GENOME_SORTED, T_out)) return -1;
    if (want_model && !c->have_params) return fail("%s: set parameters first", who);
    const int T = *T_out, M = c->M;
    if (n_seg > T) return fail("%s: segment list longer than the genome order (%d segments, %d positions)", who, n_seg, T);
    OrientBuf& o = c->orient;
    if (o.M != M || n_seg > o.cap || !o.sc) {
        const int cap = std::max(std::max(n_seg, o.M == M ? o.cap : 0), 1);
        free_orient_buffers(c);
        DALLOC(o.seg, (size_t)M);
        DALLOC(o.first, (size_t)cap);
        DALLOC(o.last, (size_t)cap);
        DALLOC(o.geo, (size_t)cap);
        DALLOC(o.bnd, (size_t)cap);
        DALLOC(o.large, (size_t)cap);
        DALLOC(o.obs, 4 * (size_t)cap);
        DALLOC(o.expq, 2 * (size_t)cap);
        DALLOC(o.sc, (size_t)ORIENT_NS);
        DALLOC(o.ctl, 2);
        o.M = M;
        o.cap = cap;
    }
    HIPCK(hipMemsetAsync(o.ctl, 0, 2 * sizeof(int), c->stream));
    HIPCK(hipMemsetAsync(o.sc, 0, ORIENT_NS * sizeof(unsigned long long), c->stream));
    if (n_seg > 0) {
        HIPCK(hipMemcpyAsync(o.first, first, (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(o.last, last, (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_orient_segments, dim3((n_seg + ORIENT_THREADS - 1) / ORIENT_THREADS), dim3(ORIENT_THREADS), 0, c->stream, o.first, o.last, n_seg, c->genome.meta, T,
                           window, wave_pairs, o.geo, o.bnd, o.large, o.ctl);
    }
    if (T > 0) hipLaunchKernelGGL(k_orient_paint, dim3((T + ORIENT_THREADS - 1) / ORIENT_THREADS), dim3(ORIENT_THREADS), 0, c->stream, o.first, o.last, n_seg, T, o.seg);
    int ctl[2] = {0, 0};
    HIPCK(hipMemcpyAsync(ctl, o.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream)); /* (the caller's list is pageable host memory) */
    if (ctl[ORIENT_CTL_ERR])
        return fail("%s: segment list malformed:%s%s%s (the segments are intervals of positions 0 .. %d, ascending, disjoint, each inside one contig)", who,
                    ctl[ORIENT_CTL_ERR] & 1 ? " an entry out of range;" : "", ctl[ORIENT_CTL_ERR] & 2 ? " not ascending and disjoint;" : "",
                    ctl[ORIENT_CTL_ERR] & 4 ? " a segment spans two contigs;" : "", T - 1);
    if (ctl[ORIENT_CTL_LARGE] < 0 || ctl[ORIENT_CTL_LARGE] > n_seg) return fail("%s: %d of %d segments listed (device error)", who, ctl[ORIENT_CTL_LARGE], n_seg);
    *n_large = ctl[ORIENT_CTL_LARGE];
    return 0;
}

/* zero + the observed pass on the library's stream */
static int orient_enqueue_observed(ig_ctx* c, int n_seg, int window, bool combine)
{
    OrientBuf& o = c->orient;
    if (n_seg > 0) HIPCK(hipMemsetAsync(o.obs, 0, 4 * (size_t)n_seg * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(o.sc, 0, ORIENT_N_OBS * sizeof(unsigned long long), c->stream));
    if (c->Z == 0) return 0;
    const int blocks = (int)std::min<long long>((c->Z + ORIENT_THREADS - 1) / ORIENT_THREADS, 4096);
    const bool narrow = c->max_count < (1 << 25); /* 64 counts fit an int */
    const dim3 grid(blocks), block(ORIENT_THREADS);
    if (combine && narrow)
        hipLaunchKernelGGL((k_orient_observed<true, int>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, o.seg, o.bnd, window, o.obs, o.sc, c->rank, c->world);
    else if (combine)
        hipLaunchKernelGGL((k_orient_observed<true, long long>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, o.seg, o.bnd, window, o.obs, o.sc, c->rank,
                           c->world);
    else
        hipLaunchKernelGGL((k_orient_observed<false, int>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, o.seg, o.bnd, window, o.obs, o.sc, c->rank, c->world);
    return 0;
}

/* the model pass: every word of expq is written by the launch that owns its segment */
static int orient_enqueue_model(ig_ctx* c, int n_seg, int n_large, long long wave_pairs)
{
    OrientBuf& o = c->orient;
    HIPCK(hipMemsetAsync(o.sc + ORIENT_DEV_MAXQ, 0, sizeof(unsigned long long), c->stream));
    if (n_seg == 0) return 0;
    hipLaunchKernelGGL((k_orient_model<64>), dim3((unsigned)(((long long)n_seg * 64 + ORIENT_THREADS - 1) / ORIENT_THREADS)), dim3(ORIENT_THREADS), 0, c->stream, c->genome.ds, o.geo,
                       o.bnd, (const int*)nullptr, n_seg, wave_pairs, c->glob, o.expq, o.sc + ORIENT_DEV_MAXQ);
    if (n_large > 0)
        hipLaunchKernelGGL((k_orient_model<ORIENT_THREADS>), dim3(n_large), dim3(ORIENT_THREADS), 0, c->stream, c->genome.ds, o.geo, o.bnd, (const int*)o.large, n_large, wave_pairs,
                           c->glob, o.expq, o.sc + ORIENT_DEV_MAXQ);
    return 0;
}

/* a class of a segment adds at most arm * (left flank + right flank) <= 2 w^2 values */
static int orient_check_model(ig_ctx* c, const char* who, int window)
{
    return check_model_values(c, who, c->orient.sc + ORIENT_DEV_MAXQ, 2ull * (unsigned long long)window * (unsigned long long)window);
}

extern "C" int ig_orientation_support(ig_ctx* c, int32_t window, int32_t model, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t* geometry,
                                      int64_t* observed, int64_t* expected_q, int64_t* scalars, int32_t* n_placed)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_orientation_support";
    if (!scalars || !n_placed || (n_seg > 0 && (!geometry || !observed))) return fail("%s: NULL output", who);
    if (model && n_seg > 0 && !expected_q) return fail("%s: NULL output (expected_q may be NULL only with model == 0)", who);
    int T = 0, n_large = 0;
    if (orient_prepare(c, who, window, model != 0, n_seg, seg_first, seg_last, ORIENT_WAVE_PAIRS, &T, &n_large)) return -1;
    if (orient_enqueue_observed(c, n_seg, window, ORIENT_SHIP_COMBINE != 0)) return -1;
    if (model) {
        if (orient_enqueue_model(c, n_seg, n_large, ORIENT_WAVE_PAIRS)) return -1;
        if (orient_check_model(c, who, window)) return -1;
    }
    OrientBuf& o = c->orient;
    long long sc[ORIENT_NS];
    HIPCK(hipMemcpyAsync(sc, o.sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    if (n_seg > 0) {
        HIPCK(hipMemcpyAsync(geometry, o.geo, (size_t)n_seg * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(observed, o.obs, 4 * (size_t)n_seg * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        if (model) HIPCK(hipMemcpyAsync(expected_q, o.expq, 2 * (size_t)n_seg * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    long long judged = 0;
    for (int k = 0; k < n_seg; k++) judged += geometry[4 * (size_t)k] == 0;
    for (int k = 0; k < ORIENT_N_OBS; k++) scalars[k] = sc[k];
    scalars[ORIENT_JUDGED] = judged;
    *n_placed = T;
    return 0;
}

extern "C" int ig_debug_orientation_support_time(ig_ctx* c, int32_t window, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t pass, int32_t form,
                                                 int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_orientation_support_time";
    if (n < 1 || !ms_n) return fail("%s: bad arguments", who);
    if (pass != ORIENT_PASS_OBSERVED && pass != ORIENT_PASS_MODEL) return fail("%s: pass 0 (observed) or 1 (model), got %d", who, pass);
    if (form < 0 || form > (pass == ORIENT_PASS_MODEL ? 2 : 1)) return fail("%s: no form %d of pass %d", who, form, pass);
    const bool model = pass == ORIENT_PASS_MODEL;
    const long long wave_pairs = !model || form == 0 ? (long long)ORIENT_WAVE_PAIRS : form == 1 ? 0x7fffffffffffffffll : -1ll;
    int T = 0, n_large = 0;
    if (orient_prepare(c, who, window, model, n_seg, seg_first, seg_last, wave_pairs, &T, &n_large)) return -1;
    OrientBuf& o = c->orient;
    std::vector<long long> h;
    if (!model) {
        if (time_repeats(c, who, n, ms_n, [&] { return orient_enqueue_observed(c, n_seg, window, form != 0); })) return -1;
        h.assign(4 * (size_t)n_seg + ORIENT_N_OBS, 0);
        if (n_seg > 0) HIPCK(hipMemcpy(h.data(), o.obs, 4 * (size_t)n_seg * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(h.data() + 4 * (size_t)n_seg, o.sc, ORIENT_N_OBS * sizeof(long long), hipMemcpyDeviceToHost));
    } else {
        if (time_repeats(c, who, n, ms_n, [&] { return orient_enqueue_model(c, n_seg, n_large, wave_pairs); })) return -1;
        if (orient_check_model(c, who, window)) return -1;
        h.assign(2 * (size_t)n_seg, 0);
        if (n_seg > 0) HIPCK(hipMemcpy(h.data(), o.expq, 2 * (size_t)n_seg * sizeof(long long), hipMemcpyDeviceToHost));
    }
    if (checksum) { /* of the last pass: every word weighted by its place: every form of a pass must agree on it */
        *checksum = (long long)weighted_checksum(h.data(), h.size());
    }
    return 0;
}
