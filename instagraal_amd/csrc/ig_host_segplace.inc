/* ig_host_segplace.inc -- part of ig_hip.hip (one translation unit; included there in order): segment placement support, where the
 * contacts say a run of bins belongs and which way round (ig_kernels_segplace.cuh; the rule: instagraal_amd/segment_placement.py). */

/* the passes ig_debug_segment_placement_time reports, in this order */
#define SEGPLACE_P_RECORDS 0
#define SEGPLACE_P_COUNT 1
#define SEGPLACE_P_ROWS 2
#define SEGPLACE_P_SCATTER 3
#define SEGPLACE_P_SORT_SHORT 4
#define SEGPLACE_P_SORT_LDS 5
#define SEGPLACE_P_SORT_LONG 6
#define SEGPLACE_P_REDUCE 7
#define SEGPLACE_P_PREFIX 8
#define SEGPLACE_P_SCAN 9
#define SEGPLACE_P_QUADRANTS 10
#define SEGPLACE_PASSES 11
#define SEGPLACE_SCALARS 9 /* ig_segment_placement's scalars: the SEGPLACE_NS of the device, then n_contigs, n_guests, n_placed */

/* the one free function of the feature: called first thing and at the end of every call, whatever happened, and by ig_destroy */
static void free_segplace_buffers(ig_ctx* c)
{
    SegPlaceBuf& p = c->segplace;
    hipFree(p.head);
    hipFree(p.incl);
    hipFree(p.htot);
    hipFree(p.rec);
    hipFree(p.ends);
    hipFree(p.first);
    hipFree(p.last);
    hipFree(p.seg_of);
    hipFree(p.recs);
    hipFree(p.err);
    hipFree(p.sc);
    rows_free(p.rows);
    hipFree(p.pre);
    hipFree(p.ptot);
    hipFree(p.out_i);
    hipFree(p.out_l);
    hipFree(p.win);
    hipFree(p.quad);
    long long forms[8];
    for (int k = 0; k < 8; k++) forms[k] = p.forms[k];
    p = SegPlaceBuf{};
    for (int k = 0; k < 8; k++) p.forms[k] = forms[k];
}

/* One call up to the device's arrays (p.out_i, p.out_l, p.quad) and the scalars: the records and the segments, the rows of the profile
 * (rows_build) from k_segplace_emit, their prefix sums, the placement support's scan over the sites, the quadrants.  The caller frees
 * everything. */
static int segplace_impl(ig_ctx* c, const char* who, int window, int min_hosts, int n_seg, const int32_t* first, const int32_t* last, float* ms,
                         long long scalars[SEGPLACE_SCALARS])
{
    SegPlaceBuf& p = c->segplace;
    for (int k = 0; k < 8; k++) p.forms[k] = 0;
    if (check_window(who, window)) return -1;
    if (min_hosts < 1 || min_hosts > 2 * window) return fail("%s: 1 <= min_hosts <= 2 * window = %d (got %d)", who, 2 * window, min_hosts);
    if (n_seg < 0) return fail("%s: segment list of %d entries", who, n_seg);
    if (n_seg > 0 && (!first || !last)) return fail("%s: NULL segment list", who);
    if (c->world != 1) return fail("%s: segment placement needs all contacts on one handle (this one holds shard %d of %d)", who, c->rank, c->world);
    int T = 0;
    if (genome_positions(c, who, GENOME_SORTED, &T)) return -1;
    if (n_seg > T) return fail("%s: segment list out of range: 0 <= first <= last < %d (%d segments)", who, T, n_seg);
    LiftTimer timer(c, ms, SEGPLACE_PASSES);
    DALLOC(p.sc, (size_t)SEGPLACE_NS);
    HIPCK(hipMemsetAsync(p.sc, 0, SEGPLACE_NS * sizeof(unsigned long long), c->stream));
    DALLOC(p.err, 1);
    HIPCK(hipMemsetAsync(p.err, 0, sizeof(int), c->stream));
    /* the records: per sub-fragment (the join support's), per position, per segment */
    long long K = 0;
    timer.begin();
    if (join_enqueue_records(c, who, T, p.head, p.incl, p.htot, p.rec, p.ends, &K)) return -1;
    const int Ki = (int)K;
    DALLOC(p.first, (size_t)n_seg);
    DALLOC(p.last, (size_t)n_seg);
    DALLOC(p.seg_of, (size_t)T);
    DALLOC(p.recs, (size_t)n_seg);
    if (n_seg > 0) {
        HIPCK(hipMemcpyAsync(p.first, first, (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(p.last, last, (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_segplace_records, dim3((n_seg + SEGPLACE_THREADS - 1) / SEGPLACE_THREADS), dim3(SEGPLACE_THREADS), 0, c->stream, p.first, p.last, n_seg,
                           c->genome.meta, p.incl, T, Ki, p.recs, p.err);
    }
    if (T > 0)
        hipLaunchKernelGGL(k_segplace_map, dim3((T + SEGPLACE_THREADS - 1) / SEGPLACE_THREADS), dim3(SEGPLACE_THREADS), 0, c->stream, p.first, p.last, n_seg, T, p.seg_of);
    timer.end(SEGPLACE_P_RECORDS);
    int err = 0;
    HIPCK(hipMemcpyAsync(&err, p.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream)); /* (the caller's list is pageable host memory) */
    if (err & 1) return fail("%s: segment list out of range: 0 <= first <= last < %d", who, T);
    if (err & 2) return fail("%s: segment list not ascending and disjoint", who);
    if (err) return fail("%s: segment list: a segment spans two contigs", who);
    /* the profile */
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (c->Z == 0) return; /* no contacts: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(c->Z)), block(SEGPLACE_THREADS);
        if (!scatter) hipLaunchKernelGGL((k_segplace_emit<false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, p.rec, p.seg_of, T, n_seg, slots, ent, n_ent, p.sc);
        else hipLaunchKernelGGL((k_segplace_emit<true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, p.rec, p.seg_of, T, n_seg, slots, ent, n_ent, p.sc);
    };
    unsigned long long sc[SEGPLACE_NS];
    auto check = [&](long long E) {
        for (int k = 0; k < SEGPLACE_NS; k++) scalars[k] = (long long)sc[k];
        scalars[6] = K;
        scalars[7] = 0;
        scalars[8] = T;
        /* the overflow guard: obs * hosts <= sum(counts) * 2 w must stay below 2^62 (a quadrant is a part of obs) */
        unsigned long long total = 0;
        for (int k = 0; k < SEGPLACE_ENTRIES; k++) {
            if (sc[k] >= 1ull << 62) return fail("%s: counts too large for this window", who);
            total += sc[k];
        }
        if (total > ((1ull << 62) - 1) / (2ull * (unsigned long long)window)) /* 2 w total >= 2^62 */
            return fail("%s: counts too large for this window (the contacts sum to %llu; times %d hosts that does not fit the 64-bit comparison)", who, total,
                        2 * window);
        if (E < 0 || E > 2 * (long long)c->Z || (E > 0 && (K < 1 || n_seg < 1)))
            return fail("%s: %lld entries of %lld contacts over %lld contigs (device error)", who, E, (long long)c->Z, K);
        if (E > 0x7fffffffll) return fail("%s: %lld entries are more than one call can sort (2^31 - 1)", who, E);
        return 0;
    };
    /* per entry, as the placement support's rows: the word itself, the long rows' scratch and their runs' items (8 bytes each), a bit,
     * and a summed entry of its own (position, count, prefix sum: 20 bytes); the quadrants and the windows are per segment, not per
     * entry */
    const RowsSpec spec = {p.sc, SEGPLACE_NS, SEGPLACE_ENTRIES, 45, "", true,
                           {SEGPLACE_P_COUNT, SEGPLACE_P_ROWS, SEGPLACE_P_SCATTER, SEGPLACE_P_SORT_SHORT, SEGPLACE_P_REDUCE}};
    long long E = 0, n_sum = 0;
    if (rows_build(c, who, p.rows, n_seg, spec, sc, check, emit, timer, p.forms, &E, &n_sum)) return -1;
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
    timer.end(SEGPLACE_P_PREFIX);
    DALLOC(p.out_i, (size_t)SEGPLACE_NI * (size_t)n_seg);
    DALLOC(p.out_l, (size_t)SEGPLACE_NL * (size_t)n_seg);
    DALLOC(p.win, (size_t)SEGPLACE_SITES * (size_t)n_seg);
    DALLOC(p.quad, (size_t)SEGPLACE_SITES * 4 * (size_t)n_seg);
    if (n_seg == 0) { /* an empty list: the class sums are the result */
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }
    /* the scan: the placement support's, over the segment records, in the form its handle setting asks for */
    const int form = c->place.form;
    const long long wave_entries = form == 1 ? (long long)0x7fffffffffffffffll : form == 2 ? -1ll : (long long)PLACE_WAVE_ENTRIES;
    const dim3 per_seg((n_seg + SEGPLACE_THREADS - 1) / SEGPLACE_THREADS);
    timer.begin();
    if (form != 2)
        hipLaunchKernelGGL((k_place_scan<1>), dim3((n_seg + PLACE_THREADS - 1) / PLACE_THREADS), dim3(PLACE_THREADS), 0, c->stream, p.recs, n_seg, r.rowptr, r.out_col, p.pre,
                           n_sum, c->genome.meta, p.incl, T, Ki, window, min_hosts, wave_entries, p.out_i, p.out_l);
    if (form != 1)
        hipLaunchKernelGGL((k_place_scan<64>), dim3((unsigned)(((long long)n_seg * 64 + PLACE_THREADS - 1) / PLACE_THREADS)), dim3(PLACE_THREADS), 0, c->stream, p.recs, n_seg,
                           r.rowptr, r.out_col, p.pre, n_sum, c->genome.meta, p.incl, T, Ki, window, min_hosts, wave_entries, p.out_i, p.out_l);
    timer.end(SEGPLACE_P_SCAN);
    /* the quadrants */
    timer.begin();
    HIPCK(hipMemsetAsync(p.quad, 0, (size_t)SEGPLACE_SITES * 4 * (size_t)n_seg * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_segplace_windows, per_seg, dim3(SEGPLACE_THREADS), 0, c->stream, p.recs, n_seg, p.out_i, p.ends, Ki, T, window, p.win,
                       p.out_i + (size_t)PLACE_NI * (size_t)n_seg);
    if (c->Z > 0)
        hipLaunchKernelGGL(k_segplace_quadrants, dim3(lift_blocks(c->Z)), dim3(SEGPLACE_THREADS), 0, c->stream, c->crow, c->cc, c->Z, p.rec, p.seg_of, T, n_seg, window, p.recs,
                           p.win, p.quad);
    timer.end(SEGPLACE_P_QUADRANTS);
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* the call, the arrays to the caller (ints: SEGPLACE_NI arrays of n_seg words, longs: SEGPLACE_NL, quadrants: n_seg * 12 words), the
 * buffers freed whatever happened */
static int segplace_call(ig_ctx* c, const char* who, int window, int min_hosts, int n_seg, const int32_t* first, const int32_t* last, float* ms, int32_t* ints,
                         int64_t* longs, int64_t* quadrants, long long scalars[SEGPLACE_SCALARS])
{
    free_segplace_buffers(c);
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    int rc = segplace_impl(c, who, window, min_hosts, n_seg, first, last, ms, scalars);
    const size_t n = (size_t)std::max(n_seg, 0);
    if (!rc && n > 0) {
        hipError_t e = hipMemcpy(ints, c->segplace.out_i, (size_t)SEGPLACE_NI * n * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(longs, c->segplace.out_l, (size_t)SEGPLACE_NL * n * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(quadrants, c->segplace.quad, (size_t)SEGPLACE_SITES * 4 * n * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail("%s: the arrays could not be read: %s", who, hipGetErrorString(e));
    }
    free_segplace_buffers(c);
    if (rc) return rc;
    long long guests = 0;
    for (size_t s = 0; s < n; s++) guests += ints[s] == 0;
    scalars[7] = guests;
    return 0;
}

extern "C" int ig_segment_placement(ig_ctx* c, int32_t window, int32_t min_hosts, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t* ints,
                                    int64_t* longs, int64_t* quadrants, int64_t scalars[9])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_segment_placement";
    if (!scalars || (n_seg > 0 && (!ints || !longs || !quadrants))) return fail("%s: NULL output", who);
    long long sc[SEGPLACE_SCALARS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (segplace_call(c, who, window, min_hosts, n_seg, seg_first, seg_last, nullptr, ints, longs, quadrants, sc)) return -1;
    for (int k = 0; k < SEGPLACE_SCALARS; k++) scalars[k] = sc[k];
    return 0;
}

extern "C" int ig_debug_segment_placement_time(ig_ctx* c, int32_t window, int32_t min_hosts, int32_t n_seg, const int32_t* seg_first, const int32_t* seg_last, int32_t n,
                                               float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_segment_placement_time";
    if (n < 1 || !ms_n) return fail("%s: bad arguments", who);
    if (n_seg < 0) return fail("%s: segment list of %d entries", who, n_seg);
    const size_t ns = (size_t)n_seg;
    std::vector<int32_t> vi((size_t)SEGPLACE_NI * ns + 1);
    std::vector<int64_t> vl((size_t)SEGPLACE_NL * ns + 1), vq((size_t)SEGPLACE_SITES * 4 * ns + 1);
    long long sc[SEGPLACE_SCALARS];
    for (int r = 0; r < n; r++)
        if (segplace_call(c, who, window, min_hosts, n_seg, seg_first, seg_last, ms_n + (size_t)r * SEGPLACE_PASSES, vi.data(), vl.data(), vq.data(), sc)) return -1;
    if (checksum) { /* of the last result: every output word -- the int32 arrays, the int64 arrays, the quadrants, the scalars -- weighted by its place */
        std::vector<long long> all(vi.begin(), vi.end() - 1);
        all.insert(all.end(), vl.begin(), vl.end() - 1);
        all.insert(all.end(), vq.begin(), vq.end() - 1);
        all.insert(all.end(), sc, sc + SEGPLACE_SCALARS);
        *checksum = (long long)weighted_checksum(all.data(), all.size());
    }
    return 0;
}
