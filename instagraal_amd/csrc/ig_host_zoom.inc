/* ig_host_zoom.inc -- part of ig_hip.hip (one translation unit; included there in order): fixed-resolution maps of the current genome
 * (ig_kernels_zoom.cuh; the rule: instagraal_amd/zoom_levels.py; DESIGN.md 4.21): the lift and the balancing's build with a caller's
 * unit per position (lift_build, ig_host_lift.inc; bal_build, ig_host_bal.inc), and the coarsening of a built, reduced level through
 * the row builder's sorts and reduction (ig_host_rows.inc). */

/* the passes of a coarsening, in this order */
#define ZOOM_P_ROWSTART 0
#define ZOOM_P_WORDS 1
#define ZOOM_P_SORT_SHORT 2
#define ZOOM_P_SORT_LDS 3
#define ZOOM_P_SORT_LONG 4
#define ZOOM_P_REDUCE 5
#define ZOOM_PASSES 6

/* a table of n words, non-decreasing and inside 0 .. n_values - 1; what: "unit table" / "coarse map" */
static int zoom_check_table(const char* who, const char* what, const int32_t* tab, int64_t n, int64_t n_values)
{
    if (n < 0 || n_values < 0) return fail("%s: the %s has %lld entries for %lld values: neither may be negative", who, what, (long long)n, (long long)n_values);
    if (n_values > 0x7fffffffll) return fail("%s: %lld units are more than 2^31 - 1 (a column is 32 bits)", who, (long long)n_values);
    if (n > 0x7fffffffll) return fail("%s: the %s has %lld entries, more than 2^31 - 1", who, what, (long long)n);
    if (n > 0 && !tab) return fail("%s: NULL %s", who, what);
    for (int64_t k = 0; k < n; k++) {
        if (tab[k] < 0 || tab[k] >= n_values) return fail("%s: the %s is out of range: entry %lld is %d, the values are 0 .. %lld", who, what, (long long)k, tab[k], (long long)n_values - 1);
        if (k > 0 && tab[k] < tab[k - 1]) return fail("%s: the %s is not monotone: entry %lld is %d behind %d", who, what, (long long)k, tab[k], tab[k - 1]);
    }
    return 0;
}

extern "C" int ig_assembly_contacts_build_units(ig_ctx* c, const int32_t* unit, int64_t n_positions, int64_t n_units, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_assembly_contacts_build_units";
    lift_release_snapshot(c); /* whatever happens, the result of an earlier build is gone */
    if (!n_entries || !scalars) return fail("%s: NULL output", who);
    if (zoom_check_table(who, "unit table", unit, n_positions, n_units)) return -1;
    static const int32_t none = 0; /* (no position: the table may be NULL, the build still wants a table to tell the level by) */
    long long sc[8];
    if (lift_build(c, who, 2, nullptr, sc, unit ? unit : &none, n_positions, n_units)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_entries = c->lift.n_entries;
    return 0;
}

extern "C" int ig_balance_build_units(ig_ctx* c, const int32_t* unit, int64_t n_positions, int64_t n_units, int32_t ignore_diags, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_balance_build_units";
    free_bal_buffers(c); /* whatever happens, the result of an earlier build is gone */
    if (!n_entries || !scalars) return fail("%s: NULL output", who);
    if (zoom_check_table(who, "unit table", unit, n_positions, n_units)) return -1;
    static const int32_t none = 0;
    long long sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (bal_build(c, who, 1, 0, ignore_diags, nullptr, sc, unit ? unit : &none, n_positions, n_units)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_entries = c->bal.n_entries;
    return 0;
}

/* a coarsened level on the device */
struct ZoomOut {
    unsigned long long* rowptr = nullptr; /* [C + 1] */
    int* col = nullptr;                   /* [n_out] */
    unsigned long long* cnt = nullptr;    /* [n_out] */
    long long n_out = 0;
};

static void zoom_free_out(ZoomOut& o)
{
    hipFree(o.rowptr);
    hipFree(o.col);
    hipFree(o.cnt);
    o = ZoomOut{};
}

/* The coarsening of the U rows (rowptr [U + 1], col and cnt [K], on the device; columns strictly ascending inside a row, inside
 * 0 .. U - 1) under d_map [U] (on the device; checked on the host: non-decreasing, inside 0 .. C - 1) into o.  t: the temporaries
 * (count, cursor, tot, sc; rowstart: the segments' starts; ent: the words; work) -- its result fields are not touched, so the
 * snapshot's own RowBuf serves; the caller frees them (rows_free_temp) and, on an error, o.  The last launches are waited for. */
static int zoom_coarsen_rows(ig_ctx* c, const char* who, RowBuf& t, const unsigned long long* rowptr, const int* col, const unsigned long long* cnt, long long U,
                             long long K, const int* d_map, long long C, LiftTimer& timer, long long forms[8], ZoomOut& o)
{
    for (int k = 0; k < 8; k++) forms[k] = 0;
    const int Ui = (int)U, Ci = (int)C;
    if (K == 0) { /* no entry: the rows, all zero, are the result */
        DALLOC(o.rowptr, (size_t)C + 1);
        HIPCK(hipMemsetAsync(o.rowptr, 0, ((size_t)C + 1) * sizeof(unsigned long long), c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }
    if (U < 1 || C < 1) return fail("%s: %lld entries in %lld rows for %lld coarse rows (inconsistent)", who, K, U, C);
    /* per fine entry: the word, the long segments' scratch and their runs' items (8 bytes each), a bit, a summed entry (12 bytes) */
    if (rows_memory_guard(who, K, 37, Ci, " (the coarsening's temporaries)")) return -1;
    if (rows_reserve(t, C)) return -1;
    DALLOC(t.rowstart, (size_t)C + 1);
    DALLOC(t.ent, (size_t)K);
    HIPCK(hipMemsetAsync(t.sc, 0, ROWS_SC_WORDS * sizeof(unsigned long long), c->stream));
    timer.begin();
    hipLaunchKernelGGL(k_zoom_rowstart, dim3((unsigned)((U + 1 + LIFT_THREADS - 1) / LIFT_THREADS)), dim3(LIFT_THREADS), 0, c->stream, rowptr, d_map, Ui, Ci, t.rowstart);
    timer.end(ZOOM_P_ROWSTART);
    if (K > 0xffffffffll) { /* the index inside a segment is the low half of a word */
        std::vector<unsigned long long> seg((size_t)C + 1);
        HIPCK(hipMemcpyAsync(seg.data(), t.rowstart, seg.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        for (long long R = 0; R < C; R++)
            if (seg[(size_t)R + 1] - seg[(size_t)R] > 0xffffffffull)
                return fail("%s: coarse row %lld takes %llu entries, more than one call can sort (2^32 - 1)", who, R, seg[(size_t)R + 1] - seg[(size_t)R]);
    }
    timer.begin();
    const long long threads = (K + SCAN_ITEMS - 1) / SCAN_ITEMS;
    hipLaunchKernelGGL(k_zoom_words, dim3((unsigned)((threads + LIFT_THREADS - 1) / LIFT_THREADS)), dim3(LIFT_THREADS), 0, c->stream, rowptr, col, d_map, Ui, K, t.rowstart,
                       t.ent);
    timer.end(ZOOM_P_WORDS);
    if (lift_sort_rows(c, who, timer, ZOOM_P_SORT_SHORT, t.rowstart, Ci, t.ent, K, c->lift.short_max, c->lift.lds_max, t.sc + ROWS_SC_CLS, t.sc + ROWS_SC_CUR, forms, t.work))
        return -1;
    if (lift_reduce_rows(c, who, timer, ZOOM_P_REDUCE, t.rowstart, Ci, t.ent, K, t.sc + ROWS_SC_HEADS, t.count, t.tot, t.work, &o.col, &o.cnt, &o.rowptr, &o.n_out, cnt))
        return -1;
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* the map to the device (*d_map: the caller frees it), then the rows */
static int zoom_coarsen_upload(ig_ctx* c, const char* who, RowBuf& t, const unsigned long long* rowptr, const int* col, const unsigned long long* cnt, long long U,
                               long long K, const int32_t* map, int** d_map, long long C, float* ms, long long forms[8], ZoomOut& o)
{
    DALLOC(*d_map, (size_t)std::max<long long>(U, 1));
    if (U > 0) HIPCK(hipMemcpyAsync(*d_map, map, (size_t)U * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    LiftTimer timer(c, ms, ZOOM_PASSES);
    return zoom_coarsen_rows(c, who, t, rowptr, col, cnt, U, K, *d_map, C, timer, forms, o);
}

extern "C" int ig_assembly_contacts_coarsen(ig_ctx* c, const int32_t* coarse_of_unit, int64_t n_units, int64_t n_coarse, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_assembly_contacts_coarsen";
    LiftBuf& l = c->lift;
    /* a refusal leaves nothing built */
    const int refused = [&]() -> int {
        if (!n_entries || !scalars) return fail("%s: NULL output", who);
        if (!l.valid) return fail("%s: nothing is built (ig_assembly_contacts_build at level 1 or ig_assembly_contacts_build_units first)", who);
        if (l.level == 0) return fail("%s: a level 0 result cannot be coarsened (packed words, 32-bit counts): build level 1 or with a unit table", who);
        if (n_units != l.n_units) return fail("%s: the coarse map is for %lld units, the built result has %lld", who, (long long)n_units, l.n_units);
        if (zoom_check_table(who, "coarse map", coarse_of_unit, n_units, n_coarse)) return -1;
        if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
        return 0;
    }();
    if (refused) {
        lift_release_snapshot(c);
        return -1;
    }
    const long long K = l.n_entries, C = n_coarse;
    ZoomOut o;
    int* d_map = nullptr;
    const int rc = zoom_coarsen_upload(c, who, l.rows, l.rows.rowptr, l.rows.out_col, l.rows.out_cnt, l.n_units, K, coarse_of_unit, &d_map, C, nullptr, l.forms, o);
    hipStreamSynchronize(c->stream);
    hipFree(d_map);
    if (l.rows.out_col) rows_free_temp(l.rows);
    else { /* (a source without entries: the temporaries were not used, and rows_free_temp tells a reduced result by out_col) */
        hipFree(l.rows.rowstart);
        l.rows.rowstart = nullptr;
    }
    if (rc) {
        zoom_free_out(o);
        lift_release_snapshot(c);
        return rc;
    }
    const long long kept = l.contacts_kept, un0 = l.unplaced[0], un1 = l.unplaced[1], placed = l.n_placed;
    rows_free_result(l.rows); /* the old entries go once the new ones stand */
    l.rows.rowptr = o.rowptr;
    l.rows.out_col = o.col;
    l.rows.out_cnt = o.cnt;
    l.level = 2;
    l.n_units = C;
    l.n_entries = o.n_out;
    const long long sc[8] = {K, K, kept, un0, un1, placed, C, o.n_out};
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_entries = o.n_out;
    return 0;
}

/* ---- tests: the coarsening over caller CSR data, on a bare handle */
extern "C" int ig_debug_zoom_coarsen(ig_ctx* c, const int64_t* rowptr, const int32_t* col, const int64_t* count, int64_t n_rows, const int32_t* coarse_of_unit,
                                     int64_t n_coarse, int64_t* n_out, int64_t forms[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_zoom_coarsen";
    DebugRows& d = c->debug_zoom;
    d.valid = false; /* whatever happens, the result of an earlier call is gone */
    if (!n_out || !forms || !rowptr) return fail("%s: NULL argument", who);
    if (n_rows < 0 || n_rows > 0x7fffffffll) return fail("%s: %lld rows: 0 .. 2^31 - 1", who, (long long)n_rows);
    if (rowptr[0] != 0) return fail("%s: rowptr starts at 0 (got %lld)", who, (long long)rowptr[0]);
    for (int64_t u = 0; u < n_rows; u++)
        if (rowptr[u + 1] < rowptr[u]) return fail("%s: rowptr decreases behind row %lld", who, (long long)u);
    const long long U = n_rows, K = rowptr[n_rows], C = n_coarse;
    if (K > 0 && (!col || !count)) return fail("%s: NULL argument", who);
    for (long long e = 0; e < K; e++)
        if (col[e] < 0 || col[e] >= U) return fail("%s: entry %lld has column %d, there are %lld rows", who, e, col[e], U);
    if (zoom_check_table(who, "coarse map", coarse_of_unit, n_rows, n_coarse)) return -1;
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    RowBuf t;
    ZoomOut o;
    unsigned long long *d_rowptr = nullptr, *d_cnt = nullptr;
    int *d_col = nullptr, *d_map = nullptr;
    long long f[8];
    const int rc = [&]() -> int {
        DALLOC(d_rowptr, (size_t)U + 1);
        DALLOC(d_col, (size_t)std::max<long long>(K, 1));
        DALLOC(d_cnt, (size_t)std::max<long long>(K, 1));
        HIPCK(hipMemcpyAsync(d_rowptr, rowptr, ((size_t)U + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        if (K > 0) {
            HIPCK(hipMemcpyAsync(d_col, col, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIPCK(hipMemcpyAsync(d_cnt, count, (size_t)K * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        }
        if (zoom_coarsen_upload(c, who, t, d_rowptr, d_col, d_cnt, U, K, coarse_of_unit, &d_map, C, nullptr, f, o)) return -1;
        d.rowptr.assign((size_t)C + 1, 0);
        d.col.assign((size_t)o.n_out, 0);
        d.count.assign((size_t)o.n_out, 0);
        d.word.clear();
        HIPCK(hipMemcpy(d.rowptr.data(), o.rowptr, d.rowptr.size() * sizeof(long long), hipMemcpyDeviceToHost));
        if (o.n_out > 0) {
            HIPCK(hipMemcpy(d.col.data(), o.col, (size_t)o.n_out * sizeof(int), hipMemcpyDeviceToHost));
            HIPCK(hipMemcpy(d.count.data(), o.cnt, (size_t)o.n_out * sizeof(long long), hipMemcpyDeviceToHost));
        }
        return 0;
    }();
    hipStreamSynchronize(c->stream);
    rows_free(t);
    zoom_free_out(o);
    hipFree(d_rowptr);
    hipFree(d_col);
    hipFree(d_cnt);
    hipFree(d_map);
    if (rc) return rc;
    d.valid = d.reduced = true;
    for (int k = 0; k < 8; k++) forms[k] = f[k];
    *n_out = (long long)d.col.size();
    return 0;
}

extern "C" int ig_debug_zoom_fetch(ig_ctx* c, int64_t* rowptr, int64_t n_rowptr, int32_t* col, int64_t* count, int64_t capacity)
{
    IG_JOIN(c);
    const DebugRows& d = c->debug_zoom;
    if (!d.valid) return fail("ig_debug_zoom_fetch: nothing is built (ig_debug_zoom_coarsen first)");
    const size_t n_out = d.col.size();
    if (!rowptr || n_rowptr < (int64_t)d.rowptr.size() || capacity < (int64_t)n_out)
        return fail("ig_debug_zoom_fetch: the result has %zu row words and %zu entries, the caller's capacities are %lld and %lld", d.rowptr.size(), n_out,
                    (long long)n_rowptr, (long long)capacity);
    if (n_out > 0 && (!col || !count)) return fail("ig_debug_zoom_fetch: NULL output");
    memcpy(rowptr, d.rowptr.data(), d.rowptr.size() * sizeof(int64_t));
    if (n_out > 0) {
        memcpy(col, d.col.data(), n_out * sizeof(int32_t));
        memcpy(count, d.count.data(), n_out * sizeof(int64_t));
    }
    return 0;
}

/* the coarsening of the resident snapshot n times, hipEvents around each pass; the snapshot is read only and every repeat's result
 * goes to buffers of its own, freed behind it: the snapshot survives */
extern "C" int ig_debug_zoom_time(ig_ctx* c, const int32_t* coarse_of_unit, int64_t n_units, int64_t n_coarse, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_zoom_time";
    LiftBuf& l = c->lift;
    if (n < 1 || !ms_n) return fail("%s: bad arguments", who);
    if (!l.valid || l.level == 0) return fail("%s: nothing to coarsen is built (ig_assembly_contacts_build at level 1 or ig_assembly_contacts_build_units first)", who);
    if (coarse_of_unit && n_units != l.n_units) return fail("%s: the coarse map is for %lld units, the built result has %lld", who, (long long)n_units, l.n_units);
    std::vector<int32_t> halves;
    if (!coarse_of_unit) { /* the default: two units to one, whatever the caller's sizes */
        n_units = l.n_units;
        halves.resize((size_t)n_units);
        for (int64_t u = 0; u < n_units; u++) halves[(size_t)u] = (int32_t)(u / 2);
        coarse_of_unit = halves.data();
        n_coarse = (n_units + 1) / 2;
    }
    if (zoom_check_table(who, "coarse map", coarse_of_unit, n_units, n_coarse)) return -1;
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    int rc = 0;
    for (int r = 0; r < n && !rc; r++) {
        RowBuf t;
        ZoomOut o;
        int* d_map = nullptr;
        long long f[8];
        rc = zoom_coarsen_upload(c, who, t, l.rows.rowptr, l.rows.out_col, l.rows.out_cnt, l.n_units, l.n_entries, coarse_of_unit, &d_map, n_coarse,
                                 ms_n + (size_t)r * ZOOM_PASSES, f, o);
        hipStreamSynchronize(c->stream);
        if (!rc && checksum && r == n - 1)
            rc = [&]() -> int { /* of the last result: the rows, then the columns, then the counts, every word weighted by its place */
                std::vector<long long> h((size_t)n_coarse + 1 + 2 * (size_t)o.n_out, 0);
                std::vector<int> col((size_t)o.n_out);
                HIPCK(hipMemcpy(h.data(), o.rowptr, ((size_t)n_coarse + 1) * sizeof(long long), hipMemcpyDeviceToHost));
                if (o.n_out > 0) {
                    HIPCK(hipMemcpy(col.data(), o.col, (size_t)o.n_out * sizeof(int), hipMemcpyDeviceToHost));
                    HIPCK(hipMemcpy(h.data() + n_coarse + 1 + o.n_out, o.cnt, (size_t)o.n_out * sizeof(long long), hipMemcpyDeviceToHost));
                }
                for (long long k = 0; k < o.n_out; k++) h[(size_t)(n_coarse + 1 + k)] = col[(size_t)k];
                *checksum = (long long)weighted_checksum(h.data(), h.size());
                return 0;
            }();
        rows_free(t);
        zoom_free_out(o);
        hipFree(d_map);
    }
    return rc;
}
