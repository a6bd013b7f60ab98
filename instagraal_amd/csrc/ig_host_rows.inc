/* ig_host_rows.inc -- part of ig_hip.hip (one translation unit; included there in order): the row builder (ig_kernels_rows.cuh):
 * the 64-bit scan, the counting sort of a feature's entries into rows, the sort of the rows, the reduction of their equal columns,
 * and RowBuf's lifetime.  The contacts in genome coordinates, join support and placement support build their rows here
 * (rows_build); the junction profile and the expected map take the scan alone. */

/* RowBuf.sc, in 64-bit words: k_lift_classify's sizes and cursors, the heads of the reduction */
#define ROWS_SC_CLS 0
#define ROWS_SC_CUR LIFT_C_WORDS
#define ROWS_SC_HEADS (ROWS_SC_CUR + 5)
#define ROWS_SC_WORDS (ROWS_SC_HEADS + 1)

/* The free device memory is asked for through a WEAK reference: a HIP runtime without hipMemGetInfo (the fake one of the host-only
 * sanitizer harness, tests/sanitize/fake_hip_runtime.cpp) still links, and the check is skipped there.  Against libamdhip64 the
 * symbol is always bound. */
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes) __attribute__((weak));

static inline int scan_chunks(long long n_words) { return (int)((n_words + SCAN_CHUNK - 1) / SCAN_CHUNK); }

/* The 64-bit inclusive prefix sums of n_arrays arrays of n words each, `stride` words apart: in -> out (in stays as it is), in three
 * steps on the library's stream; tot: n_arrays * scan_chunks(n) words of scratch. */
static void scan64_enqueue(ig_ctx* c, const unsigned long long* in, unsigned long long* out, long long stride, int n, int n_arrays,
                           unsigned long long* tot)
{
    const int chunks = scan_chunks(n);
    hipLaunchKernelGGL(k_scan64_totals, dim3(chunks, n_arrays), dim3(SCAN_THREADS), 0, c->stream, in, stride, n, tot);
    hipLaunchKernelGGL(k_scan64_tops, dim3(n_arrays), dim3(SCAN_THREADS), 0, c->stream, tot, chunks);
    hipLaunchKernelGGL(k_scan64_apply, dim3(chunks, n_arrays), dim3(SCAN_THREADS), 0, c->stream, in, out, stride, n, tot);
}

/* ---- RowBuf's three parts and their free functions: a feature's lifetime rule is which of them it calls, and when */

/* what one build needed and its result does not (behind a reduction the sorted entries are such) */
static void rows_free_temp(RowBuf& r)
{
    hipFree(r.rowstart);
    r.rowstart = nullptr;
    if (r.out_col) {
        hipFree(r.ent);
        r.ent = nullptr;
    }
    LiftWork& w = r.work;
    hipFree(w.short_rows);
    hipFree(w.lds_items);
    hipFree(w.run_items);
    hipFree(w.long_rows);
    hipFree(w.scratch);
    hipFree(w.bits);
    hipFree(w.rtot);
    w = LiftWork{};
}

static void rows_free_result(RowBuf& r)
{
    hipFree(r.rowptr);
    hipFree(r.ent);
    hipFree(r.out_col);
    hipFree(r.out_cnt);
    r.rowptr = r.ent = r.out_cnt = nullptr;
    r.out_col = nullptr;
}

static void rows_free_reserve(RowBuf& r)
{
    hipFree(r.count);
    hipFree(r.cursor);
    hipFree(r.tot);
    hipFree(r.sc);
    r.count = r.cursor = r.tot = r.sc = nullptr;
    r.cap = -1;
}

static void rows_free(RowBuf& r)
{
    rows_free_temp(r);
    rows_free_result(r);
    rows_free_reserve(r);
}

/* count, cursor, tot and sc for builds of up to U rows: grow-only, so a feature that reserves its largest build once keeps them from
 * call to call */
static int rows_reserve(RowBuf& r, long long U)
{
    if (U <= r.cap) return 0;
    rows_free_reserve(r);
    DALLOC(r.count, (size_t)U + 2);
    DALLOC(r.cursor, (size_t)U + 2);
    DALLOC(r.tot, (size_t)scan_chunks(U + 2));
    DALLOC(r.sc, (size_t)ROWS_SC_WORDS);
    r.cap = U;
    return 0;
}

/* hipEvents around a pass where its time was asked for (ms: n_passes floats, or null): every feature that builds rows times its
 * passes through one */
struct LiftTimer {
    ig_ctx* c;
    float* ms;
    hipEvent_t a = nullptr, b = nullptr;
    LiftTimer(ig_ctx* ctx, float* out, int n_passes) : c(ctx), ms(out)
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

/* what n_ent entries of U rows need at the most, before anything is allocated by their number: per entry entry_bytes (the word
 * itself, the long rows' scratch and their runs' items, a bit, and what the feature makes of an entry), per row the lists of the
 * three forms.  hint: the end of the message */
static int rows_memory_guard(const char* who, long long n_ent, size_t entry_bytes, int U, const char* hint)
{
    const unsigned long long need = (unsigned long long)n_ent * entry_bytes + (unsigned long long)(U + 1) * (8 + sizeof(LiftItem) + sizeof(LiftLong)) + (1ull << 20);
    size_t free_b = ~(size_t)0, total_b = 0;
    if (&hipMemGetInfo != nullptr) HIPCK(hipMemGetInfo(&free_b, &total_b));
    if (need > (unsigned long long)free_b) return fail("%s: %lld entries need %llu bytes of device memory, %zu are free%s", who, n_ent, need, free_b, hint);
    return 0;
}

/* The sort of every row by column in one of three forms: k_lift_classify builds the work lists in `w`, then one launch per form.
 * rowstart: [U + 1]; ent: [K] entries; short_set, lds_set: the handle's limits (0: the default); d_cls, d_cur: LIFT_C_WORDS and 5
 * zeroed words on the device; forms: the LIFT_C_* words for the host.  The times go to the passes pass0 (short), pass0 + 1 (lds),
 * pass0 + 2 (long). */
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

/* The runs of equal columns inside a row become one entry each: heads per chunk, their scan, the sums; the heads per row, their
 * scan.  d_heads: a zeroed word on the device; count: [U + 1] words, tot: the scan's totals (both
 * scratch).  Allocates the result (*out_col, *out_cnt: [*n_out]; *rowptr: [U + 1]); everything is enqueued, the caller waits.
 * gather (the coarsening, ig_host_zoom.inc): the low half of an entry is its index inside its row, and what its run sums is
 * gather[rowstart + index], a 64-bit count (k_zoom_reduce); null: the low half is the count itself (k_lift_reduce). */
static int lift_reduce_rows(ig_ctx* c, const char* who, LiftTimer& timer, int pass, const unsigned long long* rowstart, int Ui, const unsigned long long* ent,
                            long long K, unsigned long long* d_heads, unsigned long long* count, unsigned long long* tot, LiftWork& w, int** out_col,
                            unsigned long long** out_cnt, unsigned long long** rowptr, long long* n_out, const unsigned long long* gather = nullptr)
{
    const long long U = Ui;
    const long long chunks = scan_chunks(K);
    DALLOC(w.bits, (size_t)(K + 31) / 32);
    DALLOC(w.rtot, (size_t)chunks);
    timer.begin();
    HIPCK(hipMemsetAsync(w.bits, 0, ((size_t)(K + 31) / 32) * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_lift_row_bits, dim3((unsigned)((U + LIFT_THREADS - 1) / LIFT_THREADS)), dim3(LIFT_THREADS), 0, c->stream, rowstart, Ui, w.bits);
    hipLaunchKernelGGL(k_lift_head_totals, dim3((unsigned)chunks), dim3(SCAN_THREADS), 0, c->stream, ent, w.bits, K, w.rtot, d_heads);
    hipLaunchKernelGGL(k_scan64_tops, dim3(1), dim3(SCAN_THREADS), 0, c->stream, w.rtot, (int)chunks);
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
    if (gather)
        hipLaunchKernelGGL(k_zoom_reduce, dim3((unsigned)chunks), dim3(SCAN_THREADS), 0, c->stream, ent, w.bits, K, w.rtot, rowstart, Ui, gather,
                           (unsigned long long)*n_out, *out_col, *out_cnt, count);
    else
        hipLaunchKernelGGL(k_lift_reduce, dim3((unsigned)chunks), dim3(SCAN_THREADS), 0, c->stream, ent, w.bits, K, w.rtot, rowstart, Ui, (unsigned long long)*n_out,
                           *out_col, *out_cnt, count);
    HIPCK(hipMemsetAsync(*rowptr, 0, sizeof(unsigned long long), c->stream));
    scan64_enqueue(c, count, *rowptr + 1, 0, Ui, 1, tot);
    timer.end(pass);
    return 0;
}

/* the passes a build's times go to (LiftTimer); sort: the short form, sort + 1: lds, sort + 2: long */
struct RowsPasses {
    int count, scan, scatter, sort, reduce;
};

/* what a feature tells rows_build about itself */
struct RowsSpec {
    const unsigned long long* d_sc; /* the feature's scalars on the device, summed by its counting pass ... */
    int n_sc, entries_word;         /* ... their number, and which of them is the number of entries */
    size_t entry_bytes;             /* the free-memory guard: bytes an entry needs at the most (0: no guard) ... */
    const char* guard_hint;         /* ... and the end of its message */
    bool reduce;                    /* sum the runs of equal columns */
    RowsPasses passes;
};

/* One build of rows into r, of a feature whose emit step is
 *   emit(bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent)
 * which launches the feature's own kernel over its input (the contacts, for the reports; with an empty input it launches nothing:
 * the input is the feature's, so is the gate): scatter = false, every entry counts for its row in slots[U + 2] (zeroed) and the
 * feature's scalars (spec.d_sc) are summed; scatter = true, slots hold the rows' cursors and every entry takes its place in
 * ent[n_ent].
 * The sequence: count, the scan to the rows' starts, the feature's scalars to h_sc[spec.n_sc] and check(entries) -- the feature's
 * own refusals, non-zero: stop --, the free-memory guard, the scatter, the sort of the rows (under the limits of
 * ig_debug_assembly_contacts_limits) and, spec.reduce, the sum of the equal columns.
 * Behind it r.rowptr holds the U + 1 rows of *n_out entries: r.ent, or (reduce) r.out_col and r.out_cnt; with no entry at all the
 * rows' starts, all zero, are the result's rows and nothing else is allocated.  forms: the LIFT_C_* words.  The last launches are
 * not waited for; on an error the caller frees r. */
template <class Check, class Emit>
static int rows_build(ig_ctx* c, const char* who, RowBuf& r, int U, const RowsSpec& spec, unsigned long long* h_sc, Check check, Emit emit, LiftTimer& timer,
                      long long forms[8], long long* n_entries, long long* n_out)
{
    const RowsPasses& p = spec.passes;
    for (int k = 0; k < 8; k++) forms[k] = 0;
    *n_entries = *n_out = 0;
    if (rows_reserve(r, U)) return -1;
    DALLOC(r.rowstart, (size_t)U + 1);
    HIPCK(hipMemsetAsync(r.sc, 0, ROWS_SC_WORDS * sizeof(unsigned long long), c->stream));
    /* count */
    timer.begin();
    HIPCK(hipMemsetAsync(r.count, 0, ((size_t)U + 2) * sizeof(unsigned long long), c->stream));
    emit(false, r.count, nullptr, 0ull);
    timer.end(p.count);
    /* the rows' starts */
    timer.begin();
    HIPCK(hipMemsetAsync(r.rowstart, 0, sizeof(unsigned long long), c->stream));
    if (U > 0) scan64_enqueue(c, r.count, r.rowstart + 1, 0, U, 1, r.tot);
    timer.end(p.scan);
    HIPCK(hipMemcpyAsync(h_sc, spec.d_sc, (size_t)spec.n_sc * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    const long long E = (long long)h_sc[spec.entries_word];
    *n_entries = E;
    if (check(E)) return -1;
    if (E == 0) { /* no entry: the rows' starts, all zero, are the result's rows */
        r.rowptr = r.rowstart;
        r.rowstart = nullptr;
        return 0;
    }
    if (spec.entry_bytes && rows_memory_guard(who, E, spec.entry_bytes, U, spec.guard_hint)) return -1;
    DALLOC(r.ent, (size_t)E);
    /* scatter */
    timer.begin();
    HIPCK(hipMemcpyAsync(r.cursor, r.rowstart, (size_t)U * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    emit(true, r.cursor, r.ent, (unsigned long long)E);
    timer.end(p.scatter);
    if (lift_sort_rows(c, who, timer, p.sort, r.rowstart, U, r.ent, E, c->lift.short_max, c->lift.lds_max, r.sc + ROWS_SC_CLS, r.sc + ROWS_SC_CUR, forms, r.work)) return -1;
    if (spec.reduce) return lift_reduce_rows(c, who, timer, p.reduce, r.rowstart, U, r.ent, E, r.sc + ROWS_SC_HEADS, r.count, r.tot, r.work, &r.out_col, &r.out_cnt, &r.rowptr, n_out);
    r.rowptr = r.rowstart; /* the rows' starts are the result's rows */
    r.rowstart = nullptr;
    *n_out = E;
    return 0;
}
