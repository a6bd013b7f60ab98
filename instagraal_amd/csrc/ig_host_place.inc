/* ig_host_place.inc -- part of ig_hip.hip (one translation unit; included there in order): placement support, where the contacts say
 * each bin belongs (ig_kernels_place.cuh; the rule: instagraal_amd/placement_support.py). */

/* the passes ig_debug_placement_support_time reports, in this order */
#define PLACE_P_RECORDS 0
#define PLACE_P_COUNT 1
#define PLACE_P_ROWS 2
#define PLACE_P_SCATTER 3
#define PLACE_P_SORT_SHORT 4
#define PLACE_P_SORT_LDS 5
#define PLACE_P_SORT_LONG 6
#define PLACE_P_REDUCE 7
#define PLACE_P_PREFIX 8
#define PLACE_P_SCAN 9
#define PLACE_PASSES 10

/* the one free function of the feature: called at the end of every call, whatever happened, and by ig_destroy.  The setting of
 * ig_debug_placement_support_form belongs to the handle and stays, and so do the last call's work-list sizes
 * (ig_debug_placement_support_forms: host words, no device memory). */
static void free_place_buffers(ig_ctx* c)
{
    PlaceBuf& p = c->place;
    hipFree(p.head);
    hipFree(p.incl);
    hipFree(p.htot);
    hipFree(p.rec);
    hipFree(p.ends);
    hipFree(p.bins);
    hipFree(p.sc);
    rows_free(p.rows);
    hipFree(p.pre);
    hipFree(p.ptot);
    hipFree(p.out_i);
    hipFree(p.out_l);
    const int form = p.form;
    long long forms[8];
    for (int k = 0; k < 8; k++) forms[k] = p.forms[k];
    p = PlaceBuf{};
    p.form = form;
    for (int k = 0; k < 8; k++) p.forms[k] = forms[k];
}

/* One call up to the device's arrays (p.out_i, p.out_l) and the scalars: the records and the bins, the rows of the profile
 * (rows_build) from k_place_emit, their prefix sums, the scan over the sites.  The caller frees everything. */
static int place_impl(ig_ctx* c, const char* who, int window, int min_hosts, float* ms, long long scalars[7])
{
    PlaceBuf& p = c->place;
    for (int k = 0; k < 8; k++) p.forms[k] = 0; /* (a call that fails reports no lists of an earlier one) */
    if (check_window(who, window)) return -1;
    if (min_hosts < 1 || min_hosts > 2 * window) return fail("%s: 1 <= min_hosts <= 2 * window = %d (got %d)", who, 2 * window, min_hosts);
    if (c->world != 1) return fail("%s: placement support needs all contacts on one handle (this one holds shard %d of %d)", who, c->rank, c->world);
    int T = 0;
    if (genome_positions(c, who, GENOME_SORTED, &T)) return -1;
    const int M = c->M, N = c->N;
    if (N < 1 || N > 2 * M + 3) return fail("%s: %d bins over %d sub-fragments (inconsistent tables)", who, N, M);
    LiftTimer timer(c, ms, PLACE_PASSES);
    DALLOC(p.sc, (size_t)PLACE_NS);
    HIPCK(hipMemsetAsync(p.sc, 0, PLACE_NS * sizeof(unsigned long long), c->stream));
    /* the records: per sub-fragment (the join support's), per bin */
    long long K = 0;
    timer.begin();
    if (join_enqueue_records(c, who, T, p.head, p.incl, p.htot, p.rec, p.ends, &K)) return -1;
    const int Ki = (int)K;
    DALLOC(p.bins, (size_t)N);
    hipLaunchKernelGGL(k_place_bins, dim3((N + PLACE_THREADS - 1) / PLACE_THREADS), dim3(PLACE_THREADS), 0, c->stream, c->st.sub_first, c->st.sl, N, M, p.rec, T, p.bins);
    timer.end(PLACE_P_RECORDS);
    /* the profile */
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (c->Z == 0) return; /* no contacts: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(c->Z)), block(PLACE_THREADS);
        if (!scatter) hipLaunchKernelGGL((k_place_emit<false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, p.rec, c->sub_tab, N, slots, ent, n_ent, p.sc);
        else hipLaunchKernelGGL((k_place_emit<true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, p.rec, c->sub_tab, N, slots, ent, n_ent, p.sc);
    };
    unsigned long long sc[PLACE_NS];
    auto check = [&](long long E) {
        for (int k = 0; k < PLACE_NS; k++) scalars[k] = (long long)sc[k];
        scalars[5] = K;
        scalars[6] = 0;
        /* the overflow guard: obs * hosts <= sum(counts) * 2 w must stay below 2^62 */
        unsigned long long total = 0;
        for (int k = 0; k < 4; k++) {
            if (sc[k] >= 1ull << 62) return fail("%s: counts too large for this window", who);
            total += sc[k];
        }
        if (total > ((1ull << 62) - 1) / (2ull * (unsigned long long)window)) /* 2 w total >= 2^62 */
            return fail("%s: counts too large for this window (the contacts sum to %llu; times %d hosts that does not fit the 64-bit comparison)", who, total,
                        2 * window);
        if (E < 0 || E > 2 * (long long)c->Z || (E & 1) || (E > 0 && (K < 1 || N < 2)))
            return fail("%s: %lld entries of %lld contacts over %lld contigs (device error)", who, E, (long long)c->Z, K);
        if (E > 0x7fffffffll) return fail("%s: %lld entries are more than one call can sort (2^31 - 1)", who, E);
        return 0;
    };
    /* per entry: the word itself, the long rows' scratch and their runs' items (8 bytes each), a bit, and a summed entry of its own
     * (position, count, prefix sum: 20 bytes) */
    const RowsSpec spec = {p.sc, PLACE_NS, PLACE_ENTRIES, 45, "", true, {PLACE_P_COUNT, PLACE_P_ROWS, PLACE_P_SCATTER, PLACE_P_SORT_SHORT, PLACE_P_REDUCE}};
    long long E = 0, n_sum = 0;
    if (rows_build(c, who, p.rows, N, spec, sc, check, emit, timer, p.forms, &E, &n_sum)) return -1;
    if (E == 0) { /* an empty profile: every row is empty */
        DALLOC(p.rows.out_col, (size_t)0);
        DALLOC(p.rows.out_cnt, (size_t)0);
    }
    const RowBuf& r = p.rows;
    /* the exclusive prefix sums of the summed counts */
    DALLOC(p.pre, (size_t)n_sum + 1);
    DALLOC(p.ptot, (size_t)scan_chunks(std::max<long long>(n_sum, 1)));
    timer.begin();
    HIPCK(hipMemsetAsync(p.pre, 0, sizeof(unsigned long long), c->stream));
    if (n_sum > 0) scan64_enqueue(c, r.out_cnt, p.pre + 1, 0, (int)n_sum, 1, p.ptot);
    timer.end(PLACE_P_PREFIX);
    /* the scan */
    DALLOC(p.out_i, (size_t)PLACE_NI * (size_t)N);
    DALLOC(p.out_l, (size_t)PLACE_NL * (size_t)N);
    const long long wave_entries = p.form == 1 ? (long long)0x7fffffffffffffffll : p.form == 2 ? -1ll : (long long)PLACE_WAVE_ENTRIES;
    timer.begin();
    if (p.form != 2)
        hipLaunchKernelGGL((k_place_scan<1>), dim3((N + PLACE_THREADS - 1) / PLACE_THREADS), dim3(PLACE_THREADS), 0, c->stream, p.bins, N, r.rowptr, r.out_col, p.pre, n_sum,
                           c->genome.meta, p.incl, T, Ki, window, min_hosts, wave_entries, p.out_i, p.out_l);
    if (p.form != 1)
        hipLaunchKernelGGL((k_place_scan<64>), dim3((unsigned)(((long long)N * 64 + PLACE_THREADS - 1) / PLACE_THREADS)), dim3(PLACE_THREADS), 0, c->stream, p.bins, N, r.rowptr,
                           r.out_col, p.pre, n_sum, c->genome.meta, p.incl, T, Ki, window, min_hosts, wave_entries, p.out_i, p.out_l);
    timer.end(PLACE_P_SCAN);
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* the call, the arrays to the caller (out_i: PLACE_NI pointers, out_l: PLACE_NL, each to N words), the buffers freed whatever happened */
static int place_call(ig_ctx* c, const char* who, int window, int min_hosts, float* ms, int32_t* const* out_i, int64_t* const* out_l, long long scalars[7])
{
    free_place_buffers(c);
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    int rc = place_impl(c, who, window, min_hosts, ms, scalars);
    const size_t N = (size_t)c->N;
    if (!rc) {
        hipError_t e = hipSuccess;
        for (int a = 0; a < PLACE_NI && e == hipSuccess; a++) e = hipMemcpy(out_i[a], c->place.out_i + (size_t)a * N, N * sizeof(int32_t), hipMemcpyDeviceToHost);
        for (int a = 0; a < PLACE_NL && e == hipSuccess; a++) e = hipMemcpy(out_l[a], c->place.out_l + (size_t)a * N, N * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail("%s: the arrays could not be read: %s", who, hipGetErrorString(e));
    }
    free_place_buffers(c);
    if (rc) return rc;
    long long guests = 0;
    for (size_t f = 0; f < N; f++) guests += out_i[0][f] == 0;
    scalars[6] = guests;
    return 0;
}

extern "C" int ig_placement_support(ig_ctx* c, int32_t window, int32_t min_hosts, int32_t* status, int32_t* contig, int32_t* offset, int32_t* n_positions,
                                    int32_t* home_hosts, int32_t* best_contig, int32_t* best_offset, int32_t* best_hosts, int32_t* second_contig,
                                    int32_t* second_offset, int32_t* second_hosts, int64_t* home_left, int64_t* home_right, int64_t* best_left, int64_t* best_right,
                                    int64_t* second_left, int64_t* second_right, int64_t scalars[7])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    int32_t* const oi[PLACE_NI] = {status, contig, offset, n_positions, home_hosts, best_contig, best_offset, best_hosts, second_contig, second_offset, second_hosts};
    int64_t* const ol[PLACE_NL] = {home_left, home_right, best_left, best_right, second_left, second_right};
    for (int a = 0; a < PLACE_NI; a++)
        if (!oi[a]) return fail("ig_placement_support: NULL output");
    for (int a = 0; a < PLACE_NL; a++)
        if (!ol[a]) return fail("ig_placement_support: NULL output");
    if (!scalars) return fail("ig_placement_support: NULL output");
    long long sc[7] = {0, 0, 0, 0, 0, 0, 0};
    if (place_call(c, "ig_placement_support", window, min_hosts, nullptr, oi, ol, sc)) return -1;
    for (int k = 0; k < 7; k++) scalars[k] = sc[k];
    return 0;
}

extern "C" int ig_debug_placement_support_form(ig_ctx* c, int32_t form)
{
    IG_JOIN(c);
    if (form < 0 || form > 2) return fail("ig_debug_placement_support_form: 0 (the default), 1 (a thread per row) or 2 (a wave per row), got %d", form);
    c->place.form = form;
    return 0;
}

extern "C" int ig_debug_placement_support_forms(ig_ctx* c, int64_t out8[8])
{
    IG_JOIN(c);
    if (!out8) return fail("ig_debug_placement_support_forms: NULL output");
    for (int k = 0; k < 8; k++) out8[k] = c->place.forms[k];
    return 0;
}

extern "C" int ig_debug_placement_support_time(ig_ctx* c, int32_t window, int32_t min_hosts, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_n) return fail("ig_debug_placement_support_time: bad arguments");
    const size_t N = (size_t)std::max(c->N, 1);
    std::vector<int32_t> vi((size_t)PLACE_NI * N);
    std::vector<int64_t> vl((size_t)PLACE_NL * N);
    int32_t* oi[PLACE_NI];
    int64_t* ol[PLACE_NL];
    for (int a = 0; a < PLACE_NI; a++) oi[a] = vi.data() + (size_t)a * N;
    for (int a = 0; a < PLACE_NL; a++) ol[a] = vl.data() + (size_t)a * N;
    long long sc[7];
    for (int r = 0; r < n; r++)
        if (place_call(c, "ig_debug_placement_support_time", window, min_hosts, ms_n + (size_t)r * PLACE_PASSES, oi, ol, sc)) return -1;
    if (checksum) { /* of the last result: every word of the arrays weighted by its place */
        std::vector<long long> all(vi.begin(), vi.end());
        all.insert(all.end(), vl.begin(), vl.end());
        *checksum = (long long)weighted_checksum(all.data(), all.size());
    }
    return 0;
}
