/* ig_host_join.inc -- part of ig_hip.hip (one translation unit; included there in order): join support, which scaffold ends the
 * contacts of the current genome would link (ig_kernels_join.cuh; the rule: instagraal_amd/join_support.py). */

/* JoinBuf.sc, in 64-bit words: the scalars of the passes over the contacts, the largest |quantised model value| */
#define JOIN_SC_MAXQ JOIN_NS
#define JOIN_SC_WORDS (JOIN_SC_MAXQ + 1)
/* the passes ig_debug_join_support_time reports, in this order */
#define JOIN_P_ENDS 0
#define JOIN_P_COUNT 1
#define JOIN_P_SCAN 2
#define JOIN_P_SCATTER 3
#define JOIN_P_SORT_SHORT 4
#define JOIN_P_SORT_LDS 5
#define JOIN_P_SORT_LONG 6
#define JOIN_P_REDUCE 7
#define JOIN_P_MODEL 8
#define JOIN_PASSES 9

/* the form of k_join_emit the builds run unless ig_debug_join_support_combine says otherwise: 1 a run of a wave's lanes with the same
 * row issues one atomic, 0 one atomic per emission (the yardstick).  The combined form ships only once its median is measured not
 * above the yardstick's at both bench shapes (tools/join_support_bench.py -> profiles/r11_join_support.json, DESIGN.md 4.14): not
 * measured yet */
#define JOIN_SHIP_COMBINE 0

/* the one free function of the feature: what a build needed, and (keep_snapshot = false) the built result.  The setting of
 * ig_debug_join_support_combine belongs to the handle and stays. */
static void free_join_buffers(ig_ctx* c, bool keep_snapshot)
{
    JoinBuf& j = c->join;
    hipFree(j.head);
    hipFree(j.incl);
    hipFree(j.htot);
    hipFree(j.rec);
    hipFree(j.sc);
    j.head = j.incl = j.htot = j.sc = nullptr;
    j.rec = nullptr;
    rows_free_temp(j.rows);
    rows_free_reserve(j.rows);
    if (keep_snapshot) return;
    rows_free_result(j.rows);
    hipFree(j.ends);
    hipFree(j.pairs);
    hipFree(j.expq);
    const int combine = j.combine;
    j = JoinBuf{};
    j.combine = combine;
}

/* The ends and the records, shared with the placement support (ig_host_place.inc): the heads of the linear placed contigs, their
 * 64-bit scan, the table per contig and one record per sub-fragment, on the library's stream behind the genome view (genome.meta,
 * genome.pix, genome.order of T placed positions: genome_positions with GENOME_SORTED).  Allocates head, incl: [T + 1]; htot: that
 * scan's chunk totals; ends: [K]; rec: [M] -- the caller's buffers, freed by the caller whatever happens.  Waits once, for K. */
static int join_enqueue_records(ig_ctx* c, const char* who, int T, unsigned long long*& head, unsigned long long*& incl, unsigned long long*& htot, int4*& rec,
                                JoinEnd*& ends, long long* K_out)
{
    const GenomeBuf& g = c->genome;
    const int M = c->M;
    long long K = 0;
    DALLOC(rec, (size_t)M);
    DALLOC(head, (size_t)T + 1);
    DALLOC(incl, (size_t)T + 1);
    DALLOC(htot, (size_t)scan_chunks(T + 1));
    if (T > 0) {
        hipLaunchKernelGGL(k_join_heads, dim3((T + JOIN_THREADS - 1) / JOIN_THREADS), dim3(JOIN_THREADS), 0, c->stream, g.meta, T, head);
        scan64_enqueue(c, head, incl, 0, T, 1, htot);
        unsigned long long n_heads = 0;
        HIPCK(hipMemcpyAsync(&n_heads, incl + (T - 1), sizeof(n_heads), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        if (n_heads > (unsigned long long)T) return fail("%s: %llu contigs over %d positions (inconsistent tables)", who, n_heads, T);
        K = (long long)n_heads;
    }
    const int Ki = (int)K; /* K <= T <= M */
    DALLOC(ends, (size_t)K);
    if (K > 0)
        hipLaunchKernelGGL(k_join_ends, dim3((T + JOIN_THREADS - 1) / JOIN_THREADS), dim3(JOIN_THREADS), 0, c->stream, g.meta, incl, T, Ki, g.order, M, c->sub_tab, c->st.LB, c->N,
                           ends);
    hipLaunchKernelGGL(k_join_records, dim3((M + JOIN_THREADS - 1) / JOIN_THREADS), dim3(JOIN_THREADS), 0, c->stream, g.pix, M, T, g.meta, incl, Ki, rec);
    *K_out = K;
    return 0;
}

/* The build, up to the snapshot's fields: the ends and the records, the rows of the links (rows_build) from k_join_emit, the model
 * over the links found.  The caller frees what it leaves behind and, on an error, the half-built snapshot. */
static int join_build_impl(ig_ctx* c, const char* who, int window, bool model, float* ms)
{
    JoinBuf& j = c->join;
    if (check_window(who, window)) return -1;
    int T = 0;
    if (genome_positions(c, who, GENOME_SORTED, &T)) return -1;
    if (model && !c->have_params) return fail("%s: set parameters first", who);
    LiftTimer timer(c, ms, JOIN_PASSES);
    DALLOC(j.sc, (size_t)JOIN_SC_WORDS);
    HIPCK(hipMemsetAsync(j.sc, 0, JOIN_SC_WORDS * sizeof(unsigned long long), c->stream));
    /* the ends */
    long long K = 0;
    timer.begin();
    if (join_enqueue_records(c, who, T, j.head, j.incl, j.htot, j.rec, j.ends, &K)) return -1;
    const int Ki = (int)K, Ui = 2 * Ki; /* K <= T <= M: the ends fit an int */
    timer.end(JOIN_P_ENDS);
    j.n_placed = T;
    j.n_contigs = K;
    /* the links */
    const bool combine = j.combine < 0 ? JOIN_SHIP_COMBINE != 0 : j.combine != 0;
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (c->Z == 0) return; /* no contacts: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(c->Z)), block(JOIN_THREADS);
        if (!scatter && combine)
            hipLaunchKernelGGL((k_join_emit<false, true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, j.rec, window, Ui, slots, ent, n_ent, j.sc, c->rank, c->world);
        else if (!scatter)
            hipLaunchKernelGGL((k_join_emit<false, false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, j.rec, window, Ui, slots, ent, n_ent, j.sc, c->rank, c->world);
        else if (combine)
            hipLaunchKernelGGL((k_join_emit<true, true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, j.rec, window, Ui, slots, ent, n_ent, j.sc, c->rank, c->world);
        else
            hipLaunchKernelGGL((k_join_emit<true, false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, j.rec, window, Ui, slots, ent, n_ent, j.sc, c->rank, c->world);
    };
    auto check = [&](long long E) {
        return E < 0 || E > 4 * (long long)c->Z || (E > 0 && K < 2) ? fail("%s: %lld entries of %lld contacts (device error)", who, E, (long long)c->Z) : 0;
    };
    /* per entry: the word itself, the long rows' scratch and their runs' items (8 bytes each), a bit, and a link of its own (column,
     * observed, pairs, expected_q: 28 bytes) */
    const RowsSpec spec = {j.sc, JOIN_NS, JOIN_ENTRIES, 53, " (a smaller window has fewer entries)", true,
                           {JOIN_P_COUNT, JOIN_P_SCAN, JOIN_P_SCATTER, JOIN_P_SORT_SHORT, JOIN_P_REDUCE}};
    unsigned long long sc[JOIN_NS];
    if (rows_build(c, who, j.rows, Ui, spec, sc, check, emit, timer, j.forms, &j.n_entries, &j.n_links)) return -1;
    const long long n_links = j.n_links;
    /* the model over the links found */
    if (model && n_links > 0) {
        DALLOC(j.pairs, (size_t)n_links);
        DALLOC(j.expq, (size_t)n_links);
        timer.begin();
        HIPCK(hipMemsetAsync(j.pairs, 0, (size_t)n_links * sizeof(unsigned long long), c->stream));
        HIPCK(hipMemsetAsync(j.expq, 0, (size_t)n_links * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL((k_join_model<1>), dim3((unsigned)((n_links + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS), 0, c->stream, j.rows.rowptr, Ui, j.rows.out_col,
                           n_links, j.ends, Ki, c->genome.ds, T, window, c->glob, j.pairs, j.expq, j.sc + JOIN_SC_MAXQ);
        hipLaunchKernelGGL((k_join_model<64>), dim3((unsigned)((n_links * 64 + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS), 0, c->stream, j.rows.rowptr, Ui,
                           j.rows.out_col, n_links, j.ends, Ki, c->genome.ds, T, window, c->glob, j.pairs, j.expq, j.sc + JOIN_SC_MAXQ);
        timer.end(JOIN_P_MODEL);
        if (check_model_sum(c, who, j.sc + JOIN_SC_MAXQ, window)) return -1;
    }
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* scalars: the eight words of join_support.SCALARS */
static int join_build(ig_ctx* c, const char* who, int window, bool model, float* ms, long long scalars[8])
{
    free_join_buffers(c, false); /* first thing, whatever happens: the result of an earlier build is gone */
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    const int rc = join_build_impl(c, who, window, model, ms);
    JoinBuf& j = c->join;
    unsigned long long sc[JOIN_NS] = {0, 0, 0, 0, 0, 0, 0};
    if (!rc && hipMemcpy(sc, j.sc, sizeof(sc), hipMemcpyDeviceToHost) != hipSuccess) {
        free_join_buffers(c, false);
        return fail("%s: the scalars could not be read", who);
    }
    free_join_buffers(c, !rc);
    if (rc) return rc;
    for (int k = 0; k < 6; k++) scalars[k] = (long long)sc[k];
    scalars[6] = j.n_contigs;
    scalars[7] = j.n_links;
    j.window = window;
    j.model = model;
    j.valid = true;
    return 0;
}

extern "C" int ig_join_support_build(ig_ctx* c, int32_t window, int32_t model, int64_t* n_ends, int64_t* n_links, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!n_ends || !n_links || !scalars) return fail("ig_join_support_build: NULL output");
    long long sc[8];
    if (join_build(c, "ig_join_support_build", window, model != 0, nullptr, sc)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_ends = 2 * c->join.n_contigs;
    *n_links = c->join.n_links;
    return 0;
}

extern "C" int ig_join_support_ends(ig_ctx* c, int32_t* first_position, int32_t* n_positions, int64_t capacity)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    JoinBuf& j = c->join;
    if (!j.valid) return fail("ig_join_support_ends: nothing is built (ig_join_support_build first)");
    if (capacity < j.n_contigs) return fail("ig_join_support_ends: the table has %lld contigs, the caller's capacity is %lld", j.n_contigs, (long long)capacity);
    if (j.n_contigs == 0) return 0;
    if (!first_position || !n_positions) return fail("ig_join_support_ends: NULL output");
    std::vector<JoinEnd> h((size_t)j.n_contigs);
    HIPCK(hipMemcpy(h.data(), j.ends, h.size() * sizeof(JoinEnd), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); k++) {
        first_position[k] = h[k].start;
        n_positions[k] = h[k].n;
    }
    return 0;
}

extern "C" int ig_join_support_rows(ig_ctx* c, int64_t* rowptr, int64_t capacity)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    JoinBuf& j = c->join;
    if (!j.valid) return fail("ig_join_support_rows: nothing is built (ig_join_support_build first)");
    if (!rowptr) return fail("ig_join_support_rows: NULL output");
    const long long words = 2 * j.n_contigs + 1;
    if (capacity < words) return fail("ig_join_support_rows: the rows need %lld words, the caller's capacity is %lld", words, (long long)capacity);
    HIPCK(hipMemcpy(rowptr, j.rows.rowptr, (size_t)words * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ig_join_support_fetch(ig_ctx* c, int64_t first, int64_t n, int32_t* col, int64_t* observed, int64_t* pairs, int64_t* expected_q)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    JoinBuf& j = c->join;
    if (!j.valid) return fail("ig_join_support_fetch: nothing is built (ig_join_support_build first)");
    if (first < 0 || n < 0 || first > j.n_links || n > j.n_links - first)
        return fail("ig_join_support_fetch: links %lld .. %lld are out of range (the result has %lld)", (long long)first, (long long)first + (long long)n, j.n_links);
    if ((pairs || expected_q) && !j.model) return fail("ig_join_support_fetch: the result was built with model = 0: it has no pairs and no expected_q");
    if (n == 0) return 0;
    if (!col || !observed) return fail("ig_join_support_fetch: NULL output");
    HIPCK(hipMemcpy(col, j.rows.out_col + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(observed, j.rows.out_cnt + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (pairs) HIPCK(hipMemcpy(pairs, j.pairs + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (expected_q) HIPCK(hipMemcpy(expected_q, j.expq + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ig_join_support_release(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    free_join_buffers(c, false);
    return 0;
}

extern "C" int ig_debug_join_support_combine(ig_ctx* c, int32_t combine)
{
    IG_JOIN(c);
    c->join.combine = combine < 0 ? -1 : combine != 0;
    return 0;
}

extern "C" int ig_debug_join_support_forms(ig_ctx* c, int64_t out8[8])
{
    IG_JOIN(c);
    if (!out8) return fail("ig_debug_join_support_forms: NULL output");
    if (!c->join.valid) return fail("ig_debug_join_support_forms: nothing is built (ig_join_support_build first)");
    for (int k = 0; k < 8; k++) out8[k] = c->join.forms[k];
    return 0;
}

extern "C" int ig_debug_join_support_time(ig_ctx* c, int32_t window, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_n) return fail("ig_debug_join_support_time: bad arguments");
    long long sc[8];
    for (int r = 0; r < n; r++)
        if (join_build(c, "ig_debug_join_support_time", window, c->have_params, ms_n + (size_t)r * JOIN_PASSES, sc)) return -1;
    if (checksum) { /* of the observed part of the last result: the rows, the columns and the counts, every word weighted by its place */
        JoinBuf& j = c->join;
        std::vector<long long> rows((size_t)(2 * j.n_contigs + 1));
        HIPCK(hipMemcpy(rows.data(), j.rows.rowptr, rows.size() * sizeof(long long), hipMemcpyDeviceToHost));
        unsigned long long s = weighted_checksum(rows.data(), rows.size()), place = rows.size() + 1; /* behind the rows: column, observed, column, ... */
        std::vector<int32_t> col((size_t)j.n_links);
        std::vector<int64_t> obs((size_t)j.n_links);
        if (ig_join_support_fetch(c, 0, j.n_links, col.data(), obs.data(), nullptr, nullptr)) return -1;
        for (size_t k = 0; k < col.size(); k++) {
            s += (unsigned long long)(long long)col[k] * place++;
            s += (unsigned long long)obs[k] * place++;
        }
        *checksum = (long long)s;
    }
    return 0;
}
