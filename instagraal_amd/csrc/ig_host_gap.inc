/* ig_host_gap.inc -- part of ig_hip.hip (one translation unit; included there in order): gap support, the distance the contacts put
 * across each join of the current genome (ig_kernels_gap.cuh; the rule: instagraal_amd/gap_support.py). */

/* the passes of ig_debug_gap_support_time */
#define GAP_PASS_OBSERVED 0   /* one atomic per word (the form that ships; no other is built) */
#define GAP_PASS_MODEL 1      /* the model pass as shipped (GAP_WAVE_TERMS) */
#define GAP_PASS_MODEL_WAVE 2 /* ... a wave per junction */
#define GAP_PASS_MODEL_WG 3   /* ... a workgroup per judged junction */

static void free_gap_buffers(ig_ctx* c)
{
    GapBuf& b = c->gap;
    hipFree(b.nj);
    hipFree(b.junc);
    hipFree(b.status);
    hipFree(b.geo);
    hipFree(b.large);
    hipFree(b.pairs);
    hipFree(b.obs);
    hipFree(b.logq);
    hipFree(b.expq);
    hipFree(b.gaps);
    hipFree(b.sc);
    hipFree(b.ctl);
    b = GapBuf{};
}

/* Argument checks, the genome view (its guards, the records by position, ds, meta and the order), the buffers, the list and the gaps
 * on the device: the list checked, status, geometry and pairs written, nj[] painted.  T: placed sub-fragments; n_large: junctions
 * listed for the workgroup form of the model pass under wave_terms.  Waits for the stream (the error word). */
static int gap_prepare(ig_ctx* c, const char* who, int window, int n_junc, const int32_t* junction, int n_gaps, const float* gaps_kb, long long wave_terms, int* T_out,
                       int* n_large)
{
    if (window < 1 || window > GAP_MAX_WINDOW) return fail("%s: 1 <= window <= %d positions (got %d)", who, GAP_MAX_WINDOW, window);
    if (n_gaps < GAP_MIN_GAPS || n_gaps > GAP_MAX_GAPS) return fail("%s: %d <= n_gaps <= %d (got %d)", who, GAP_MIN_GAPS, GAP_MAX_GAPS, n_gaps);
    if (!gaps_kb) return fail("%s: NULL gaps", who);
    if (gaps_kb[0] != 0.0f) return fail("%s: gaps: the first gap is 0", who);
    for (int k = 0; k < n_gaps; k++) {
        if (ig_isnanf(gaps_kb[k]) || ig_isinff(gaps_kb[k])) return fail("%s: gaps: entry %d is not finite", who, k);
        if (k > 0 && !(gaps_kb[k] > gaps_kb[k - 1])) return fail("%s: gaps: not strictly ascending at entry %d", who, k);
    }
    if (n_junc < 1) return fail("%s: junction list of %d entries (at least one junction)", who, n_junc);
    if (!junction) return fail("%s: NULL junction list", who);
    if (genome_positions(c, who, GENOME_RECORDS | GENOME_SORTED, T_out)) return -1;
    if (c->Z == 0) return fail("%s: no contacts", who);
    if (!c->have_params) return fail("%s: set parameters first", who);
    const int T = *T_out, M = c->M;
    if (n_junc > T) return fail("%s: junction list longer than the genome order (%d junctions, %d positions)", who, n_junc, T);
    GapBuf& b = c->gap;
    const size_t words = (size_t)n_junc * (size_t)n_gaps;
    if (b.M != M || n_junc > b.cap || words > b.cap_words || !b.sc) {
        const int cap = std::max(n_junc, b.M == M ? b.cap : 0);
        const size_t cap_words = std::max(words, b.M == M ? b.cap_words : (size_t)0);
        free_gap_buffers(c);
        DALLOC(b.nj, (size_t)M);
        DALLOC(b.junc, (size_t)cap);
        DALLOC(b.status, (size_t)cap);
        DALLOC(b.geo, (size_t)cap);
        DALLOC(b.large, (size_t)cap);
        DALLOC(b.pairs, (size_t)cap);
        DALLOC(b.obs, (size_t)cap);
        DALLOC(b.logq, cap_words);
        DALLOC(b.expq, cap_words);
        DALLOC(b.gaps, (size_t)GAP_MAX_GAPS);
        DALLOC(b.sc, (size_t)GAP_NS);
        DALLOC(b.ctl, 2);
        b.M = M;
        b.cap = cap;
        b.cap_words = cap_words;
    }
    HIPCK(hipMemsetAsync(b.ctl, 0, 2 * sizeof(int), c->stream));
    HIPCK(hipMemsetAsync(b.sc, 0, GAP_NS * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemcpyAsync(b.junc, junction, (size_t)n_junc * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(b.gaps, gaps_kb, (size_t)n_gaps * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gap_junctions, dim3((n_junc + GAP_THREADS - 1) / GAP_THREADS), dim3(GAP_THREADS), 0, c->stream, b.junc, n_junc, c->genome.meta, c->genome.order,
                       c->sub_tab, M, T, window, n_gaps, wave_terms, b.status, b.geo, b.pairs, b.large, b.ctl);
    if (T > 0) hipLaunchKernelGGL(k_gap_paint, dim3((T + GAP_THREADS - 1) / GAP_THREADS), dim3(GAP_THREADS), 0, c->stream, b.junc, n_junc, T, b.nj);
    int ctl[2] = {0, 0};
    HIPCK(hipMemcpyAsync(ctl, b.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream)); /* (the caller's list is pageable host memory) */
    if (ctl[GAP_CTL_ERR])
        return fail("%s: junction list malformed:%s%s%s (the junctions are positions 1 .. %d, strictly ascending, each between two positions of one contig)", who,
                    ctl[GAP_CTL_ERR] & 1 ? " an entry out of range;" : "", ctl[GAP_CTL_ERR] & 2 ? " not strictly ascending;" : "",
                    ctl[GAP_CTL_ERR] & 4 ? " a junction on a contig boundary;" : "", T - 1);
    if (ctl[GAP_CTL_LARGE] < 0 || ctl[GAP_CTL_LARGE] > n_junc) return fail("%s: %d of %d junctions listed (device error)", who, ctl[GAP_CTL_LARGE], n_junc);
    *n_large = ctl[GAP_CTL_LARGE];
    return 0;
}

/* zero + the observed pass on the library's stream */
static int gap_enqueue_observed(ig_ctx* c, int n_junc, int n_gaps, int window)
{
    GapBuf& b = c->gap;
    HIPCK(hipMemsetAsync(b.obs, 0, (size_t)n_junc * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(b.logq, 0, (size_t)n_junc * (size_t)n_gaps * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(b.sc, 0, GAP_N_OBS * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(b.sc + GAP_DEV_MAXL, 0, sizeof(unsigned long long), c->stream));
    const int blocks = (int)std::min<long long>((c->Z + GAP_THREADS - 1) / GAP_THREADS, 4096);
    hipLaunchKernelGGL(k_gap_observed, dim3(blocks), dim3(GAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, c->genome.rec, b.nj, b.gaps, n_gaps, window, c->glob, b.obs, b.logq,
                       b.sc, c->rank, c->world);
    return 0;
}

/* the model pass: every word of expq is written by the launch that owns its junction */
static int gap_enqueue_model(ig_ctx* c, int n_junc, int n_gaps, int window, int n_large, long long wave_terms)
{
    GapBuf& b = c->gap;
    HIPCK(hipMemsetAsync(b.sc + GAP_DEV_MAXE, 0, sizeof(unsigned long long), c->stream));
    constexpr int PER = GAP_THREADS / 64; /* junctions per workgroup of the wave form */
    hipLaunchKernelGGL((k_gap_model<64>), dim3((n_junc + PER - 1) / PER), dim3(GAP_THREADS), 0, c->stream, c->genome.ds, b.junc, b.status, b.geo, b.pairs, (const int*)nullptr,
                       n_junc, b.gaps, n_gaps, window, wave_terms, c->glob, b.expq, b.sc + GAP_DEV_MAXE);
    if (n_large > 0)
        hipLaunchKernelGGL((k_gap_model<GAP_THREADS>), dim3(n_large), dim3(GAP_THREADS), 0, c->stream, c->genome.ds, b.junc, b.status, b.geo, b.pairs, (const int*)b.large,
                           n_large, b.gaps, n_gaps, window, wave_terms, c->glob, b.expq, b.sc + GAP_DEV_MAXE);
    return 0;
}

/* the second guard: a word of log_q adds at most max_j observed[j] counts times the largest |quantised log| */
static int gap_check_log(const char* who, unsigned long long max_l, unsigned long long max_obs)
{
    if (max_obs > 0 && max_l > ((1ull << 62) - 1) / max_obs) /* max_l * max_obs >= 2^62 */
        return fail("%s: too many contacts across one junction for this model (%llu contacts, the largest |log10| %.6g: their product does not fit the 64-bit sum)", who,
                    max_obs, (double)max_l / IG_QSCALE);
    return 0;
}

extern "C" int ig_gap_support(ig_ctx* c, int32_t window, int32_t model, int32_t n_junc, const int32_t* junction, int32_t n_gaps, const float* gaps_kb, int32_t* status,
                              int32_t* geometry, int64_t* observed, int64_t* pairs, int64_t* log_q, int64_t* expected_q, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_gap_support";
    if (!status || !geometry || !observed || !pairs || !log_q || !scalars) return fail("%s: NULL output", who);
    if (model && !expected_q) return fail("%s: NULL output (expected_q may be NULL only with model == 0)", who);
    int T = 0, n_large = 0;
    if (gap_prepare(c, who, window, n_junc, junction, n_gaps, gaps_kb, GAP_WAVE_TERMS, &T, &n_large)) return -1;
    if (gap_enqueue_observed(c, n_junc, n_gaps, window)) return -1;
    if (model) {
        if (gap_enqueue_model(c, n_junc, n_gaps, window, n_large, GAP_WAVE_TERMS)) return -1;
        if (check_model_sum(c, who, c->gap.sc + GAP_DEV_MAXE, window)) return -1;
    }
    GapBuf& b = c->gap;
    const size_t nj = (size_t)n_junc, words = nj * (size_t)n_gaps;
    /* everything comes to host memory of this frame first: the caller's arrays are written only behind the last check */
    unsigned long long sc[GAP_NS];
    std::vector<int> h_status(nj), h_geo(4 * nj);
    std::vector<long long> h_obs(nj), h_pairs(nj), h_log(words), h_exp(model ? words : 0);
    HIPCK(hipMemcpyAsync(sc, b.sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_status.data(), b.status, nj * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_geo.data(), b.geo, nj * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_obs.data(), b.obs, nj * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_pairs.data(), b.pairs, nj * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_log.data(), b.logq, words * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (model) HIPCK(hipMemcpyAsync(h_exp.data(), b.expq, words * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    unsigned long long max_obs = 0;
    long long judged = 0;
    const std::vector<int>& canon = c->genome.canon;
    for (size_t k = 0; k < nj; k++) {
        max_obs = std::max(max_obs, (unsigned long long)h_obs[k]);
        judged += h_status[k] == 0;
        const int bin = h_geo[4 * k];
        if (bin < 0 || (size_t)bin >= canon.size()) return fail("%s: junction %d lies in no bin (device error)", who, junction[k]);
        h_geo[4 * k] = canon[(size_t)bin]; /* the device wrote the bin at position j: the contig's canonical id is the host's */
    }
    if (gap_check_log(who, sc[GAP_DEV_MAXL], max_obs)) return -1;
    memcpy(status, h_status.data(), nj * sizeof(int));
    memcpy(geometry, h_geo.data(), 4 * nj * sizeof(int));
    memcpy(observed, h_obs.data(), nj * sizeof(long long));
    memcpy(pairs, h_pairs.data(), nj * sizeof(long long));
    memcpy(log_q, h_log.data(), words * sizeof(long long));
    if (model) memcpy(expected_q, h_exp.data(), words * sizeof(long long));
    for (int k = 0; k < GAP_N_OBS; k++) scalars[k] = (long long)sc[k];
    scalars[GAP_JUDGED] = judged;
    scalars[GAP_PLACED] = T;
    return 0;
}

extern "C" int ig_model_values_host(const float params[8], const float* s, int64_t n, int64_t* e_q, int64_t* l_q)
{
    if (!params || n < 0 || (n > 0 && (!s || !e_q || !l_q))) return fail("ig_model_values_host: bad arguments");
    ig_params p;
    memcpy(&p, params, sizeof(p)); /* (eight floats in the order of ig_params) */
    for (int64_t k = 0; k < n; k++) {
        const float e = ig_rippe(s[k], p, ig_tab());
        e_q[k] = ig_quantize((double)e);
        l_q[k] = ig_quantize(ig_log10((double)e, ig_tab()));
    }
    return 0;
}

extern "C" int ig_debug_gap_support_time(ig_ctx* c, int32_t window, int32_t n_junc, const int32_t* junction, int32_t n_gaps, const float* gaps_kb, int32_t pass, int32_t n,
                                         float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_gap_support_time";
    if (n < 1 || !ms_n) return fail("%s: bad arguments", who);
    if (pass < GAP_PASS_OBSERVED || pass > GAP_PASS_MODEL_WG) return fail("%s: pass 0 (observed), 1 (model), 2 (model, a wave per junction) or 3 (model, a workgroup), got %d", who, pass);
    const long long wave_terms = pass == GAP_PASS_MODEL_WAVE ? 0x7fffffffffffffffll : pass == GAP_PASS_MODEL_WG ? -1ll : (long long)GAP_WAVE_TERMS;
    int T = 0, n_large = 0;
    if (gap_prepare(c, who, window, n_junc, junction, n_gaps, gaps_kb, wave_terms, &T, &n_large)) return -1;
    GapBuf& b = c->gap;
    const size_t nj = (size_t)n_junc, words = nj * (size_t)n_gaps;
    std::vector<long long> h;
    if (pass == GAP_PASS_OBSERVED) {
        if (time_repeats(c, who, n, ms_n, [&] { return gap_enqueue_observed(c, n_junc, n_gaps, window); })) return -1;
        h.assign(nj + words + GAP_NS, 0);
        HIPCK(hipMemcpy(h.data(), b.obs, nj * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(h.data() + nj, b.logq, words * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(h.data() + nj + words, b.sc, GAP_NS * sizeof(long long), hipMemcpyDeviceToHost));
        unsigned long long max_obs = 0;
        for (size_t k = 0; k < nj; k++) max_obs = std::max(max_obs, (unsigned long long)h[k]);
        if (gap_check_log(who, (unsigned long long)h[nj + words + GAP_DEV_MAXL], max_obs)) return -1;
        h.resize(nj + words + GAP_N_OBS); /* (the checksum: the arrays and the words the pass owns) */
    } else {
        if (time_repeats(c, who, n, ms_n, [&] { return gap_enqueue_model(c, n_junc, n_gaps, window, n_large, wave_terms); })) return -1;
        if (check_model_sum(c, who, b.sc + GAP_DEV_MAXE, window)) return -1;
        h.assign(words, 0);
        HIPCK(hipMemcpy(h.data(), b.expq, words * sizeof(long long), hipMemcpyDeviceToHost));
    }
    if (checksum) { /* of the last pass: every word weighted by its place: every form of a pass must agree on it */
        *checksum = (long long)weighted_checksum(h.data(), h.size());
    }
    return 0;
}
