/* ig_host_law.inc -- part of ig_hip.hip (one translation unit; included there in order): the distance law of the current genome
 * (ig_kernels_law.cuh; the rule: instagraal_amd/distance_law.py). */

/* LawBuf.out, in 64-bit words: the observed histogram and the observed pass's scalars, the pairs histogram and the pairs pass's
 * scalars (each pass owns its half: the pairs half can be redone alone) */
#define LAW_OUT_OBS 0
#define LAW_OUT_OSC (LAW_MAX_BINS)
#define LAW_OUT_PAIRS (LAW_MAX_BINS + LAW_NS)
#define LAW_OUT_PSC (2 * LAW_MAX_BINS + LAW_NS)
#define LAW_OUT_WORDS (2 * (LAW_MAX_BINS + LAW_NS))

static void free_law_buffers(ig_ctx* c)
{
    hipFree(c->law.edges);
    hipFree(c->law.out);
    hipFree(c->law.flag);
    c->law = LawBuf{};
}

/* Argument checks, then the records of both passes (the genome view's) and the edges on the device. */
static int law_prepare(ig_ctx* c, const char* who, const float* edges, int n_edges, bool want_pairs, int* T_out)
{
    if (!edges) return fail("%s: edges is NULL", who);
    if (n_edges < 2 || n_edges > LAW_MAX_EDGES) return fail("%s: 2 <= n_edges <= %d (got %d)", who, LAW_MAX_EDGES, n_edges);
    for (int i = 0; i < n_edges; i++) {
        if (!(edges[i] - edges[i] == 0.0f)) return fail("%s: edge %d is not finite", who, i);
        if (i && edges[i] < edges[i - 1]) return fail("%s: the edges are not sorted (edge %d < edge %d)", who, i, i - 1);
    }
    /* (the records' position is read for its sign only) */
    if (genome_positions(c, who, GENOME_RECORDS | (want_pairs ? GENOME_SORTED : 0u), T_out)) return -1;
    LawBuf& l = c->law;
    if (!l.flag) { /* (the last of the three: a build-up that failed half way starts again) */
        free_law_buffers(c);
        DALLOC(l.edges, (size_t)LAW_MAX_EDGES);
        DALLOC(l.out, (size_t)LAW_OUT_WORDS);
        DALLOC(l.flag, 1);
    }
    HIPCK(hipMemcpyAsync(c->law.edges, edges, (size_t)n_edges * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream)); /* (`edges` is the caller's pageable memory) */
    return 0;
}

/* zero + the observed pass on the library's stream */
static int law_enqueue_observed(ig_ctx* c, int n_edges, bool privatised)
{
    LawBuf& l = c->law;
    HIPCK(hipMemsetAsync(l.out + LAW_OUT_OBS, 0, (size_t)(LAW_MAX_BINS + LAW_NS) * sizeof(unsigned long long), c->stream));
    if (c->Z == 0) return 0;
    /* a workgroup zeroes and flushes a histogram of its own: no more of them than keep every CU busy */
    const int blocks = (int)std::min<long long>((c->Z + LAW_THREADS - 1) / LAW_THREADS, 2048);
    const size_t lds = law_lds_bytes(n_edges);
    if (privatised)
        hipLaunchKernelGGL((k_law_observed<true>), dim3(blocks), dim3(LAW_THREADS), lds, c->stream, c->crow, c->cc, c->Z, c->genome.rec, l.edges, n_edges,
                           l.out + LAW_OUT_OBS, l.out + LAW_OUT_OSC, c->rank, c->world);
    else
        hipLaunchKernelGGL((k_law_observed<false>), dim3(blocks), dim3(LAW_THREADS), lds, c->stream, c->crow, c->cc, c->Z, c->genome.rec, l.edges, n_edges,
                           l.out + LAW_OUT_OBS, l.out + LAW_OUT_OSC, c->rank, c->world);
    return 0;
}

/* zero + the pairs pass */
static int law_enqueue_pairs(ig_ctx* c, int T, int n_edges, bool brute)
{
    LawBuf& l = c->law;
    HIPCK(hipMemsetAsync(l.out + LAW_OUT_PAIRS, 0, (size_t)(LAW_MAX_BINS + LAW_NS) * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(l.flag, 0, sizeof(int), c->stream));
    if (T == 0) return 0;
    const int blocks = (T + LAW_THREADS - 1) / LAW_THREADS;
    const size_t lds = law_lds_bytes(n_edges);
    if (brute)
        hipLaunchKernelGGL((k_law_pairs<true>), dim3(blocks), dim3(LAW_THREADS), lds, c->stream, c->genome.ds, c->genome.meta, T, l.edges, n_edges, l.out + LAW_OUT_PAIRS,
                           l.out + LAW_OUT_PSC, l.flag);
    else
        hipLaunchKernelGGL((k_law_pairs<false>), dim3(blocks), dim3(LAW_THREADS), lds, c->stream, c->genome.ds, c->genome.meta, T, l.edges, n_edges, l.out + LAW_OUT_PAIRS,
                           l.out + LAW_OUT_PSC, l.flag);
    return 0;
}

/* the pairs pass; should dist decrease somewhere inside a contig (the run form's assumption), once more by brute force */
static int law_run_pairs(ig_ctx* c, int T, int n_edges)
{
    if (law_enqueue_pairs(c, T, n_edges, false)) return -1;
    int flag = 0;
    HIPCK(hipMemcpyAsync(&flag, c->law.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (flag) {
        if (law_enqueue_pairs(c, T, n_edges, true)) return -1;
        HIPCK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int ig_distance_law(ig_ctx* c, const float* edges, int32_t n_edges, int64_t* observed, int64_t* pairs, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!observed || !scalars) return fail("ig_distance_law: NULL output");
    int T = 0;
    if (law_prepare(c, "ig_distance_law", edges, n_edges, pairs != nullptr, &T)) return -1;
    if (law_enqueue_observed(c, n_edges, true)) return -1;
    if (pairs && law_run_pairs(c, T, n_edges)) return -1;
    std::vector<long long> h(LAW_OUT_WORDS, 0);
    HIPCK(hipMemcpyAsync(h.data(), c->law.out, (size_t)(pairs ? LAW_OUT_WORDS : LAW_MAX_BINS + LAW_NS) * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    const int nb = n_edges - 1;
    for (int b = 0; b < nb; b++) observed[b] = h[LAW_OUT_OBS + b];
    if (pairs)
        for (int b = 0; b < nb; b++) pairs[b] = h[LAW_OUT_PAIRS + b];
    for (int k = 0; k < LAW_NS; k++) scalars[k] = h[LAW_OUT_OSC + k];
    for (int k : {LAW_OOR_PAIRS, LAW_TRANS_PAIRS, LAW_RING_PAIRS, LAW_PLACED_PAIRS}) scalars[k] = pairs ? h[LAW_OUT_PSC + k] : -1;
    if (pairs) scalars[LAW_TRANS_PAIRS] = (long long)T * (long long)(T - 1) / 2 - scalars[LAW_PLACED_PAIRS];
    return 0;
}

extern "C" int ig_debug_distance_law_time(ig_ctx* c, const float* edges, int32_t n_edges, int32_t privatised, int32_t n, float* ms_observed_n,
                                          float* ms_pairs_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_observed_n) return fail("ig_debug_distance_law_time: bad arguments");
    int T = 0;
    if (law_prepare(c, "ig_debug_distance_law_time", edges, n_edges, ms_pairs_n != nullptr, &T)) return -1;
    const char* who = "ig_debug_distance_law_time";
    if (time_repeats(c, who, n, ms_observed_n, [&] { return law_enqueue_observed(c, n_edges, privatised != 0); })) return -1;
    if (ms_pairs_n && time_repeats(c, who, n, ms_pairs_n, [&] { return law_enqueue_pairs(c, T, n_edges, false); })) return -1;
    if (checksum) { /* of the last observed pass, every word weighted by its place: both forms of the kernel must agree on it */
        std::vector<long long> h(LAW_MAX_BINS + LAW_NS);
        HIPCK(hipMemcpy(h.data(), c->law.out, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
        *checksum = (long long)weighted_checksum(h.data(), h.size()); /* (the bins behind the last edge are 0: law_enqueue_observed zeroes them all) */
    }
    return 0;
}
