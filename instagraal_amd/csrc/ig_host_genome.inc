/* ig_host_genome.inc -- part of ig_hip.hip (one translation unit; included there in order): the genome view (GenomeBuf;
 * ig_kernels_genome.cuh), the tables of the current genome every report starts from, and the small helpers the reports over it
 * share (the window check, the model pass's overflow guard, the event-timed repeats and the checksum of the ig_debug_*_time entry
 * points). */

static void free_genome_buffers(ig_ctx* c)
{
    GenomeBuf& g = c->genome;
    hipFree(g.base);
    hipFree(g.pix);
    hipFree(g.order);
    hipFree(g.err);
    hipFree(g.rec);
    hipFree(g.ds);
    hipFree(g.meta);
    g = GenomeBuf{};
}

/* binning rule: bin = max(1, ceil(T / max_side)) positions per pixel, side = ceil(T / bin) pixels */
static void map_binning(long long T, long long max_side, int* bin, int* side)
{
    const long long b = std::max<long long>(1, (T + max_side - 1) / max_side);
    *bin = (int)b;
    *side = (int)((T + b - 1) / b);
}

/* what a caller wants of the view besides genome.base and genome.pix */
#define GENOME_ORDER 1u   /* genome.order */
#define GENOME_RECORDS 2u /* genome.rec: read by the passes over the contacts, so the contacts must be uploaded */
#define GENOME_SORTED 4u  /* genome.ds, genome.meta by position (with the order) */

struct GenomeDims {
    int T = 0;             /* placed sub-fragments: the positions of the genome order */
    int bin = 1, side = 0; /* positions per pixel, pixels (map_binning) */
};

/* The view of the current genome on the device: the pixel table under max_side and what `want` names.
 * Contigs in ascending order of their canonical id (what ig_download_state returns, CL:2715-2881; the reference walks np.unique of
 * its contig ids, CL:2563-2567), a contig only if every one of its bins is active (CL:2571); inside a contig the rank of a
 * sub-fragment is Tables.cp[s].y.  The numbering of the contigs is the host's (canonical_ids: a stable sort of the contig heads by
 * length, as ig_download_state does it) on the N-length state; everything M-length happens in k_map_pixels on the live tables.
 * The refusals carry the entry point's name (who).  The pixel table is waited for (its error word); k_law_records and k_law_sorted
 * are enqueued on the library's stream behind it and not waited for. */
static int genome_view(ig_ctx* c, const char* who, long long max_side, unsigned want, GenomeDims* dims)
{
    if ((want & GENOME_RECORDS) && !c->have_contacts) return fail("%s: upload the contacts first", who);
    if (!c->have_state || !c->have_sub) return fail("%s: the sub-fragment table and a state are required", who);
    if (c->nuis_in_flight) return fail("%s: a nuisance step is in flight (ig_nuis_end first)", who);
    if (c->chain_busy) return fail("%s: a chain is in flight (ig_nuis_chain_end first)", who);
    const size_t n = (size_t)c->N;
    const int M = c->M;
    HIPCK(hipStreamSynchronize(c->stream));
    std::vector<int> host(17 * n);
    HIPCK(hipMemcpy(host.data(), c->st_block, 17 * n * sizeof(int), hipMemcpyDeviceToHost));
    const int *pos = &host[0], *cid = &host[2 * n], *L = &host[7 * n], *SL = &host[8 * n], *activ = &host[15 * n];
    std::vector<int> ids;
    int nc = 0;
    canonical_ids(pos, cid, L, n, ids, &nc);
    std::vector<long long> first((size_t)nc + 1, 0); /* sub-fragments of contig id, then its first position (-1: not placed) */
    std::vector<char> placed((size_t)nc, 1);
    for (size_t f = 0; f < n; f++) {
        if (ids[f] < 0 || ids[f] >= nc) return fail("%s: a bin belongs to no contig head (inconsistent state)", who);
        if (pos[f] == 0) first[(size_t)ids[f]] = SL[f];
        if (activ[f] != 1) placed[(size_t)ids[f]] = 0;
    }
    long long T = 0;
    for (int k = 0; k < nc; k++) {
        const long long len = first[(size_t)k];
        first[(size_t)k] = placed[(size_t)k] ? T : -1;
        if (placed[(size_t)k]) T += len;
    }
    if (T > M) return fail("%s: the placed contigs hold %lld sub-fragments, the table has %d (inconsistent state)", who, T, M);
    std::vector<int> base(n);
    for (size_t f = 0; f < n; f++) base[f] = (int)first[(size_t)ids[f]];
    GenomeBuf& g = c->genome;
    if (g.N != c->N || g.M != M) {
        free_genome_buffers(c);
        DALLOC(g.base, n);
        DALLOC(g.pix, (size_t)M);
        DALLOC(g.order, (size_t)M);
        DALLOC(g.err, 1);
        DALLOC(g.rec, (size_t)M);
        DALLOC(g.ds, (size_t)M);
        DALLOC(g.meta, (size_t)M);
        g.N = c->N;
        g.M = M;
    }
    g.canon = ids; /* (host: the canonical id of every bin's contig, for the reports that name contigs) */
    dims->T = (int)T;
    map_binning(T, max_side, &dims->bin, &dims->side);
    const bool order = (want & (GENOME_ORDER | GENOME_SORTED)) != 0;
    HIPCK(hipMemcpyAsync(g.base, base.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemsetAsync(g.err, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_map_pixels, dim3((M + 255) / 256), dim3(256), 0, c->stream, c->sub_tab, c->tab, g.base, M, (int)T, dims->bin, g.pix, order ? g.order : nullptr,
                       g.err);
    int err = 0;
    HIPCK(hipMemcpyAsync(&err, g.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream)); /* (`base` is pageable host memory of this frame) */
    if (err) return fail("%s: the coordinate tables and the state disagree (a rank beyond its contig)", who);
    if (want & GENOME_RECORDS) hipLaunchKernelGGL(k_law_records, dim3((M + 255) / 256), dim3(256), 0, c->stream, c->tab, g.pix, M, g.rec);
    if ((want & GENOME_SORTED) && T > 0) hipLaunchKernelGGL(k_law_sorted, dim3((int)((T + 255) / 256)), dim3(256), 0, c->stream, c->tab, g.order, M, (int)T, g.ds, g.meta);
    return 0;
}

/* the view with one position per pixel (max_side = M >= T), so that genome.pix[s] and genome.rec[s].w are the POSITION of
 * sub-fragment s in the genome order, and the order itself; T: the positions */
static int genome_positions(ig_ctx* c, const char* who, unsigned want, int* T)
{
    GenomeDims d;
    if (genome_view(c, who, std::max(c->M, 1), want | GENOME_ORDER, &d)) return -1;
    *T = d.T;
    return 0;
}

/* the window of the junction profile, join support and placement support, in positions */
static int check_window(const char* who, int window)
{
    if (window < 1 || window > JUNC_MAX_WINDOW) return fail("%s: 1 <= window <= %d positions (got %d)", who, JUNC_MAX_WINDOW, window);
    return 0;
}

/* the overflow guard of a model pass that left the largest |quantised value| it saw in *d_maxq and adds at most n_values of them into
 * one word.  Waits for the stream. */
static int check_model_values(ig_ctx* c, const char* who, const unsigned long long* d_maxq, unsigned long long n_values)
{
    unsigned long long max_q = 0;
    HIPCK(hipMemcpyAsync(&max_q, d_maxq, sizeof(max_q), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (max_q > ((1ull << 62) - 1) / n_values) /* max_q * n_values >= 2^62 */
        return fail("%s: model value too large for this window (the largest value, %.6g, times %llu pairs does not fit the 64-bit sum)", who,
                    (double)max_q / IG_QSCALE, n_values);
    return 0;
}

/* ... of k_junc_model and k_join_model: a junction or a link adds at most w (w + 1) / 2 values (< 2^20) */
static int check_model_sum(ig_ctx* c, const char* who, const unsigned long long* d_maxq, int window)
{
    return check_model_values(c, who, d_maxq, (unsigned long long)window * (unsigned long long)(window + 1) / 2);
}

/* the checksum of the ig_debug_*_time entry points: the n words of h, each weighted by its place (1, 2, ...), modulo 2^64: every
 * form of a pass must agree on it */
static unsigned long long weighted_checksum(const long long* h, size_t n)
{
    unsigned long long s = 0;
    for (size_t k = 0; k < n; k++) s += (unsigned long long)h[k] * (unsigned long long)(k + 1);
    return s;
}

/* n repetitions of enqueue() -- launches on the library's stream, non-zero: stop -- between two events, waited for each: the
 * milliseconds go to ms[r] (ms may be null).  The events are destroyed whatever happens. */
template <class Enqueue>
static int time_repeats(ig_ctx* c, const char* who, int n, float* ms, Enqueue enqueue)
{
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    int rc = e == hipSuccess ? 0 : fail("%s: %s", who, hipGetErrorString(e));
    for (int r = 0; r < n && !rc; r++) {
        e = hipEventRecord(a, c->stream);
        rc = enqueue();
        if (e == hipSuccess) e = hipEventRecord(b, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        float t = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
        if (ms) ms[r] = t;
        if (e != hipSuccess && !rc) rc = fail("%s: %s", who, hipGetErrorString(e));
    }
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
    return rc;
}
