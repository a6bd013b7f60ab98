/* ig_host_lift.inc -- part of ig_hip.hip (one translation unit; included there in order): the contacts in the coordinates of the
 * current genome (ig_kernels_lift.cuh; the rule: instagraal_amd/assembly_contacts.py). */

/* LiftBuf.sc, in 64-bit words: the scalars of the passes over the contacts, k_lift_classify's sizes and cursors, the heads of level 1 */
#define LIFT_SC_CLS LIFT_NS
#define LIFT_SC_CUR (LIFT_SC_CLS + LIFT_C_WORDS)
#define LIFT_SC_HEADS (LIFT_SC_CUR + 5)
#define LIFT_SC_WORDS (LIFT_SC_HEADS + 1)
/* the passes ig_debug_assembly_contacts_time reports, in this order */
#define LIFT_P_COUNT 0
#define LIFT_P_SCAN 1
#define LIFT_P_SCATTER 2
#define LIFT_P_SORT_SHORT 3
#define LIFT_P_SORT_LDS 4
#define LIFT_P_SORT_LONG 5
#define LIFT_P_REDUCE 6
#define LIFT_PASSES 7

static void lift_work_free(LiftWork& w)
{
    hipFree(w.short_rows);
    hipFree(w.lds_items);
    hipFree(w.run_items);
    hipFree(w.long_rows);
    hipFree(w.scratch);
    hipFree(w.bits);
    hipFree(w.rtot);
    w = LiftWork{};
}

/* what one build needed and its result does not */
static void lift_free_temp(ig_ctx* c)
{
    LiftBuf& l = c->lift;
    hipFree(l.rowstart);
    l.rowstart = nullptr;
    lift_work_free(l.work);
}

static void lift_release_snapshot(ig_ctx* c)
{
    LiftBuf& l = c->lift;
    hipFree(l.rowptr);
    hipFree(l.ent);
    hipFree(l.out_col);
    hipFree(l.out_cnt);
    l.rowptr = l.ent = l.out_cnt = nullptr;
    l.out_col = nullptr;
    l.valid = false;
    l.n_units = l.n_entries = 0;
}

/* everything but the settings of ig_debug_assembly_contacts_limits / _combine, which belong to the handle */
static void free_lift_buffers(ig_ctx* c)
{
    LiftBuf& l = c->lift;
    lift_free_temp(c);
    lift_release_snapshot(c);
    hipFree(l.key);
    hipFree(l.head);
    hipFree(l.incl);
    hipFree(l.count);
    hipFree(l.cursor);
    hipFree(l.tot);
    hipFree(l.sc);
    const int short_max = l.short_max, lds_max = l.lds_max;
    const bool no_combine = l.no_combine;
    l = LiftBuf{};
    l.short_max = short_max;
    l.lds_max = lds_max;
    l.no_combine = no_combine;
}

/* hipEvents around a pass where its time was asked for (ms: n_passes floats, or null) */
struct LiftTimer {
    ig_ctx* c;
    float* ms;
    hipEvent_t a = nullptr, b = nullptr;
    LiftTimer(ig_ctx* ctx, float* out, int n_passes = LIFT_PASSES) : c(ctx), ms(out)
    {
        if (!ms) return;
        for (int p = 0; p < n_passes; p++) ms[p] = 0.0f;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) ms = nullptr;
    }
    ~LiftTimer()
    {
        if (a) hipEventDestroy(a);
        if (b) hipEventDestroy(b);
    }
    void begin()
    {
        if (ms) hipEventRecord(a, c->stream);
    }
    void end(int pass)
    {
        if (!ms) return;
        float t = 0.0f;
        if (hipEventRecord(b, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess)
            ms[pass] += t;
    }
};

static inline int lift_blocks(long long n) { return (int)std::min<long long>((n + LIFT_THREADS - 1) / LIFT_THREADS, 4096); }

/* The sort of every row by column in one of three forms, shared with the join support (ig_host_join.inc): k_lift_classify builds
 * the work lists in `w`, then one launch per form.  rowstart: [U + 1]; ent: [K] entries; short_max, lds_max: the handle's limits (0:
 * the default); cls, cur: LIFT_C_WORDS and 5 zeroed words on the device; forms: the LIFT_C_* words for the host.  The times go to
 * the passes pass0 (short), pass0 + 1 (lds), pass0 + 2 (long). */
static int lift_sort_rows(ig_ctx* c, const char* who, LiftTimer& timer, int pass0, const unsigned long long* rowstart, int Ui, unsigned long long* ent,
                          long long K, int short_set, int lds_set, unsigned long long* d_cls, unsigned long long* d_cur, long long forms[8], LiftWork& w)
{
    const long long U = Ui;
    const int short_max = std::min(short_set > 0 ? short_set : LIFT_SHORT_CAP, LIFT_SHORT_CAP);
    const int lds_max = std::min(lds_set > 0 ? lds_set : LIFT_LDS_CAP, LIFT_LDS_CAP);
    const dim3 rows_grid((unsigned)((U + LIFT_THREADS - 1) / LIFT_THREADS));
    hipLaunchKernelGGL((k_lift_classify<false>), rows_grid, dim3(LIFT_THREADS), 0, c->stream, rowstart, Ui, short_max, lds_max, d_cls, d_cur, nullptr, nullptr, nullptr,
                       nullptr);
    unsigned long long cls[LIFT_C_WORDS];
    HIPCK(hipMemcpyAsync(cls, d_cls, sizeof(cls), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < LIFT_C_WORDS; k++) forms[k] = (long long)cls[k];
    const long long n_short = forms[LIFT_C_SHORT_ROWS], n_lds = forms[LIFT_C_LDS_ROWS], n_long = forms[LIFT_C_LONG_ROWS];
    const long long n_runs = forms[LIFT_C_RUNS], long_ent = forms[LIFT_C_LONG_ENT], max_long = forms[LIFT_C_MAX_LONG];
    if (n_short < 0 || n_lds < 0 || n_long < 0 || n_runs < 0 || long_ent < 0 || max_long < 0 || n_short + n_lds + n_long > U || long_ent > K || n_runs > K || max_long > K)
        return fail("%s: the work lists do not add up (device error)", who);
    DALLOC(w.short_rows, (size_t)n_short);
    DALLOC(w.lds_items, (size_t)n_lds);
    DALLOC(w.run_items, (size_t)n_runs);
    DALLOC(w.long_rows, (size_t)n_long);
    DALLOC(w.scratch, (size_t)long_ent);
    hipLaunchKernelGGL((k_lift_classify<true>), rows_grid, dim3(LIFT_THREADS), 0, c->stream, rowstart, Ui, short_max, lds_max, d_cls, d_cur, w.short_rows, w.lds_items,
                       w.run_items, w.long_rows);
    /* one launch per form */
    timer.begin();
    if (n_short > 0)
        hipLaunchKernelGGL(k_lift_sort_wave, dim3((unsigned)((n_short + LIFT_THREADS / 64 - 1) / (LIFT_THREADS / 64))), dim3(LIFT_THREADS), 0, c->stream, w.short_rows,
                           (int)n_short, rowstart, ent);
    timer.end(pass0);
    timer.begin();
    if (n_lds > 0) hipLaunchKernelGGL(k_lift_sort_lds, dim3((unsigned)n_lds), dim3(LIFT_THREADS), 0, c->stream, w.lds_items, ent);
    timer.end(pass0 + 1);
    timer.begin();
    if (n_long > 0) {
        if (n_runs > 0) hipLaunchKernelGGL(k_lift_sort_lds, dim3((unsigned)n_runs), dim3(LIFT_THREADS), 0, c->stream, w.run_items, ent);
        const dim3 grid((unsigned)n_long, (unsigned)std::min<long long>(std::max<long long>((max_long + 4 * LIFT_THREADS - 1) / (4 * LIFT_THREADS), 1), 1024));
        int to_scratch = 1;
        for (long long width = lds_max; width < max_long; width *= 2, to_scratch ^= 1)
            hipLaunchKernelGGL(k_lift_merge, grid, dim3(LIFT_THREADS), 0, c->stream, w.long_rows, ent, w.scratch, width, to_scratch);
        if (!to_scratch) /* the merged rows are in the scratch buffer: a step with nothing left to merge copies them back */
            hipLaunchKernelGGL(k_lift_merge, grid, dim3(LIFT_THREADS), 0, c->stream, w.long_rows, ent, w.scratch, max_long, 0);
    }
    timer.end(pass0 + 2);
    return 0;
}

/* The runs of equal columns inside a row become one entry each, shared with the join support: heads per chunk, their scan, the
 * sums; the heads per row, their scan.  d_heads: a zeroed word on the device; count: [U + 1] words, tot: the scan's totals (both
 * scratch).  Allocates the result (*out_col, *out_cnt: [*n_out]; *rowptr: [U + 1]); everything is enqueued, the caller waits. */
static int lift_reduce_rows(ig_ctx* c, const char* who, LiftTimer& timer, int pass, const unsigned long long* rowstart, int Ui, const unsigned long long* ent,
                            long long K, unsigned long long* d_heads, unsigned long long* count, unsigned long long* tot, LiftWork& w, int** out_col,
                            unsigned long long** out_cnt, unsigned long long** rowptr, long long* n_out)
{
    const long long U = Ui;
    const long long chunks = (K + JUNC_CHUNK - 1) / JUNC_CHUNK;
    DALLOC(w.bits, (size_t)(K + 31) / 32);
    DALLOC(w.rtot, (size_t)chunks);
    timer.begin();
    HIPCK(hipMemsetAsync(w.bits, 0, ((size_t)(K + 31) / 32) * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_lift_row_bits, dim3((unsigned)((U + LIFT_THREADS - 1) / LIFT_THREADS)), dim3(LIFT_THREADS), 0, c->stream, rowstart, Ui, w.bits);
    hipLaunchKernelGGL(k_lift_head_totals, dim3((unsigned)chunks), dim3(JUNC_THREADS), 0, c->stream, ent, w.bits, K, w.rtot, d_heads);
    hipLaunchKernelGGL(k_junc_scan_tops, dim3(1), dim3(JUNC_THREADS), 0, c->stream, w.rtot, (int)chunks);
    unsigned long long heads = 0;
    HIPCK(hipMemcpyAsync(&heads, d_heads, sizeof(heads), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (heads < 1 || heads > (unsigned long long)K) return fail("%s: %llu distinct entries of %lld (device error)", who, heads, K);
    *n_out = (long long)heads;
    DALLOC(*out_col, (size_t)*n_out);
    DALLOC(*out_cnt, (size_t)*n_out);
    DALLOC(*rowptr, (size_t)U + 1);
    HIPCK(hipMemsetAsync(*out_cnt, 0, (size_t)*n_out * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(count, 0, ((size_t)U + 1) * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_lift_reduce, dim3((unsigned)chunks), dim3(JUNC_THREADS), 0, c->stream, ent, w.bits, K, w.rtot, rowstart, Ui, (unsigned long long)*n_out,
                       *out_col, *out_cnt, count);
    HIPCK(hipMemsetAsync(*rowptr, 0, sizeof(unsigned long long), c->stream));
    scan64_enqueue(c, count, *rowptr + 1, 0, Ui, 1, tot);
    timer.end(pass);
    return 0;
}

/* The build, up to the snapshot's fields.  The caller frees what it leaves behind (lift_free_temp) and, on an error, the half-built
 * snapshot. */
static int lift_build_impl(ig_ctx* c, const char* who, int level, float* ms)
{
    LiftBuf& l = c->lift;
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    int T = 0, bin = 1, side = 0;
    /* max_side = M >= T: one position per pixel, so map.pix is the position itself (as law_records) */
    if (map_prepare(c, who, std::max(c->M, 1), true, &T, &bin, &side)) return -1;
    const int M = c->M;
    if (l.M != M) {
        free_lift_buffers(c);
        DALLOC(l.key, (size_t)M);
        DALLOC(l.head, (size_t)M + 1);
        DALLOC(l.incl, (size_t)M + 1);
        DALLOC(l.count, (size_t)M + 1);
        DALLOC(l.cursor, (size_t)M + 1);
        DALLOC(l.tot, (size_t)junc_chunks(M + 2));
        DALLOC(l.sc, (size_t)LIFT_SC_WORDS);
        l.M = M;
    }
    LiftTimer timer(c, ms);
    /* the units */
    long long U = T;
    if (level == 1 && T > 0) {
        hipLaunchKernelGGL(k_lift_heads, dim3((T + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->sub_tab, c->map.order, T, l.head);
        scan64_enqueue(c, l.head, l.incl, 0, T, 1, l.tot);
        unsigned long long n_units = 0;
        HIPCK(hipMemcpyAsync(&n_units, l.incl + (T - 1), sizeof(n_units), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        if (n_units < 1 || n_units > (unsigned long long)T) return fail("%s: %llu units over %d positions (inconsistent tables)", who, n_units, T);
        U = (long long)n_units;
    }
    hipLaunchKernelGGL(k_lift_keys, dim3((M + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->map.pix, M, T, level == 1 ? l.incl : nullptr,
                       l.key);
    const int Ui = (int)U;
    /* count */
    timer.begin();
    HIPCK(hipMemsetAsync(l.count, 0, ((size_t)U + 1) * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(l.sc, 0, LIFT_SC_WORDS * sizeof(unsigned long long), c->stream));
    if (c->Z > 0) {
        if (l.no_combine)
            hipLaunchKernelGGL((k_lift_pass<false, false>), dim3(lift_blocks(c->Z)), dim3(LIFT_THREADS), 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, l.count, nullptr,
                               0ull, l.sc, c->rank, c->world);
        else
            hipLaunchKernelGGL((k_lift_pass<false, true>), dim3(lift_blocks(c->Z)), dim3(LIFT_THREADS), 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, l.count, nullptr,
                               0ull, l.sc, c->rank, c->world);
    }
    timer.end(LIFT_P_COUNT);
    /* the rows' starts */
    DALLOC(l.rowstart, (size_t)U + 1);
    timer.begin();
    HIPCK(hipMemsetAsync(l.rowstart, 0, sizeof(unsigned long long), c->stream));
    if (U > 0) scan64_enqueue(c, l.count, l.rowstart + 1, 0, Ui, 1, l.tot);
    timer.end(LIFT_P_SCAN);
    unsigned long long sc[LIFT_NS];
    HIPCK(hipMemcpyAsync(sc, l.sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    const long long K = (long long)sc[LIFT_ENTRIES_KEPT];
    if (K < 0 || K > c->Z) return fail("%s: %lld entries kept of %lld (device error)", who, K, (long long)c->Z);
    for (int k = 0; k < 8; k++) l.forms[k] = 0;
    if (K > 0) {
        DALLOC(l.ent, (size_t)K);
        /* scatter */
        timer.begin();
        HIPCK(hipMemcpyAsync(l.cursor, l.rowstart, (size_t)U * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
        if (l.no_combine)
            hipLaunchKernelGGL((k_lift_pass<true, false>), dim3(lift_blocks(c->Z)), dim3(LIFT_THREADS), 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, l.cursor, l.ent,
                               (unsigned long long)K, l.sc, c->rank, c->world);
        else
            hipLaunchKernelGGL((k_lift_pass<true, true>), dim3(lift_blocks(c->Z)), dim3(LIFT_THREADS), 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, l.cursor, l.ent,
                               (unsigned long long)K, l.sc, c->rank, c->world);
        timer.end(LIFT_P_SCATTER);
        if (lift_sort_rows(c, who, timer, LIFT_P_SORT_SHORT, l.rowstart, Ui, l.ent, K, l.short_max, l.lds_max, l.sc + LIFT_SC_CLS, l.sc + LIFT_SC_CUR, l.forms,
                           l.work))
            return -1;
    }
    long long n_out = K;
    if (level == 1 && K > 0) {
        if (lift_reduce_rows(c, who, timer, LIFT_P_REDUCE, l.rowstart, Ui, l.ent, K, l.sc + LIFT_SC_HEADS, l.count, l.tot, l.work, &l.out_col, &l.out_cnt,
                             &l.rowptr, &n_out))
            return -1;
        HIPCK(hipStreamSynchronize(c->stream));
        hipFree(l.ent);
        l.ent = nullptr;
    } else { /* the rows' starts are the result's rows */
        l.rowptr = l.rowstart;
        l.rowstart = nullptr;
    }
    HIPCK(hipStreamSynchronize(c->stream));
    l.level = level;
    l.n_units = U;
    l.n_entries = n_out;
    l.n_placed = T;
    return 0;
}

/* scalars: the eight words of assembly_contacts.SCALARS */
static int lift_build(ig_ctx* c, const char* who, int level, float* ms, long long scalars[8])
{
    lift_release_snapshot(c); /* whatever happens, the result of an earlier build is gone */
    if (level != 0 && level != 1) return fail("%s: level is 0 (sub-fragments) or 1 (bins), got %d", who, level);
    const int rc = lift_build_impl(c, who, level, ms);
    lift_free_temp(c);
    if (rc) {
        lift_release_snapshot(c);
        return rc;
    }
    LiftBuf& l = c->lift;
    unsigned long long sc[LIFT_NS];
    if (hipMemcpy(sc, l.sc, sizeof(sc), hipMemcpyDeviceToHost) != hipSuccess) {
        lift_release_snapshot(c);
        return fail("%s: the scalars could not be read", who);
    }
    for (int k = 0; k < LIFT_NS; k++) scalars[k] = (long long)sc[k];
    scalars[5] = l.n_placed;
    scalars[6] = l.n_units;
    scalars[7] = l.n_entries;
    l.valid = true;
    return 0;
}

extern "C" int ig_assembly_contacts_build(ig_ctx* c, int32_t level, int64_t* n_units, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!n_units || !n_entries || !scalars) return fail("ig_assembly_contacts_build: NULL output");
    long long sc[8];
    if (lift_build(c, "ig_assembly_contacts_build", level, nullptr, sc)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_units = c->lift.n_units;
    *n_entries = c->lift.n_entries;
    return 0;
}

extern "C" int ig_assembly_contacts_rows(ig_ctx* c, int64_t* rowptr, int64_t capacity)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    LiftBuf& l = c->lift;
    if (!l.valid) return fail("ig_assembly_contacts_rows: nothing is built (ig_assembly_contacts_build first)");
    if (!rowptr) return fail("ig_assembly_contacts_rows: NULL output");
    if (capacity < l.n_units + 1) return fail("ig_assembly_contacts_rows: the rows need %lld words, the caller's capacity is %lld", l.n_units + 1, (long long)capacity);
    HIPCK(hipMemcpy(rowptr, l.rowptr, ((size_t)l.n_units + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ig_assembly_contacts_fetch(ig_ctx* c, int64_t first, int64_t n, int32_t* col, int64_t* count)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    LiftBuf& l = c->lift;
    if (!l.valid) return fail("ig_assembly_contacts_fetch: nothing is built (ig_assembly_contacts_build first)");
    if (first < 0 || n < 0 || first > l.n_entries || n > l.n_entries - first)
        return fail("ig_assembly_contacts_fetch: entries %lld .. %lld are out of range (the result has %lld)", (long long)first, (long long)first + (long long)n, l.n_entries);
    if (n == 0) return 0;
    if (!col || !count) return fail("ig_assembly_contacts_fetch: NULL output");
    if (l.level == 1) {
        HIPCK(hipMemcpy(col, l.out_col + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(count, l.out_cnt + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        return 0;
    }
    const int64_t piece = 1 << 22; /* the packed words come through a staging buffer of 32 MiB */
    std::vector<unsigned long long> stage((size_t)std::min(n, piece));
    for (int64_t o = 0; o < n; o += piece) {
        const int64_t m = std::min(piece, n - o);
        HIPCK(hipMemcpy(stage.data(), l.ent + first + o, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < m; k++) {
            col[o + k] = (int32_t)(stage[(size_t)k] >> 32);
            count[o + k] = (int64_t)(int32_t)(unsigned)(stage[(size_t)k] & 0xffffffffull);
        }
    }
    return 0;
}

extern "C" int ig_assembly_contacts_release(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    lift_release_snapshot(c);
    return 0;
}

extern "C" int ig_debug_assembly_contacts_limits(ig_ctx* c, int32_t short_max, int32_t lds_max)
{
    IG_JOIN(c);
    if (short_max < 0 || lds_max < 0) return fail("ig_debug_assembly_contacts_limits: a limit is 0 (the default) or positive (got %d, %d)", short_max, lds_max);
    c->lift.short_max = short_max;
    c->lift.lds_max = lds_max;
    return 0;
}

extern "C" int ig_debug_assembly_contacts_combine(ig_ctx* c, int32_t combine)
{
    IG_JOIN(c);
    c->lift.no_combine = combine == 0;
    return 0;
}

extern "C" int ig_debug_assembly_contacts_forms(ig_ctx* c, int64_t out8[8])
{
    IG_JOIN(c);
    if (!out8) return fail("ig_debug_assembly_contacts_forms: NULL output");
    if (!c->lift.valid) return fail("ig_debug_assembly_contacts_forms: nothing is built (ig_assembly_contacts_build first)");
    for (int k = 0; k < 8; k++) out8[k] = c->lift.forms[k];
    return 0;
}

extern "C" int ig_debug_assembly_contacts_time(ig_ctx* c, int32_t level, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_n) return fail("ig_debug_assembly_contacts_time: bad arguments");
    long long sc[8];
    for (int r = 0; r < n; r++)
        if (lift_build(c, "ig_debug_assembly_contacts_time", level, ms_n + (size_t)r * LIFT_PASSES, sc)) return -1;
    if (checksum) { /* of the last result: the rows, the columns and the counts, every word weighted by its place */
        LiftBuf& l = c->lift;
        unsigned long long s = 0, place = 1;
        std::vector<long long> rows((size_t)l.n_units + 1);
        HIPCK(hipMemcpy(rows.data(), l.rowptr, rows.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (long long v : rows) s += (unsigned long long)v * place++;
        const int64_t piece = 1 << 22;
        std::vector<int32_t> col((size_t)std::min<int64_t>(l.n_entries, piece));
        std::vector<int64_t> cnt(col.size());
        for (int64_t o = 0; o < l.n_entries; o += piece) {
            const int64_t m = std::min<int64_t>(piece, l.n_entries - o);
            if (ig_assembly_contacts_fetch(c, o, m, col.data(), cnt.data())) return -1;
            for (int64_t k = 0; k < m; k++) {
                s += (unsigned long long)(long long)col[(size_t)k] * place++;
                s += (unsigned long long)cnt[(size_t)k] * place++;
            }
        }
        *checksum = (long long)s;
    }
    return 0;
}

/* tests: the one way to a state with a contig that is not placed (ig_upload_state refuses inactive bins: dead in the reference).
 * Nothing but the genome order (map_prepare) reads `activ`. */
extern "C" int ig_debug_set_bin_active(ig_ctx* c, int32_t bin, int32_t active)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->have_state) return fail("ig_debug_set_bin_active: upload a state first");
    if (bin < 0 || bin >= c->N) return fail("ig_debug_set_bin_active: bin %d of %d", bin, c->N);
    if (c->nuis_in_flight || c->chain_busy) return fail("ig_debug_set_bin_active: a nuisance step or a chain is in flight");
    HIPCK(hipStreamSynchronize(c->stream));
    const int v = active ? 1 : 0;
    HIPCK(hipMemcpy(c->st_block + 15 * (size_t)c->N + (size_t)bin, &v, sizeof(int), hipMemcpyHostToDevice));
    return 0;
}
