/* ig_host_balsnap.inc -- part of ig_hip.hip (one translation unit; included there in order): the balancing's rows from a built map
 * (ig_kernels_balsnap.cuh; the rule: entries_of_rows, instagraal_amd/balance.py; DESIGN.md 4.29).  A second BUILD, not a second
 * balancer: it fills c->bal's rows from the handle's snapshot (LiftBuf: ig_assembly_contacts_build[_units], _coarsen,
 * ig_pairs_pixels_build) through the row builder (rows_build, ig_host_rows.inc) without its reduction; ig_balance_rows, _fetch, _run
 * and _release (ig_host_bal.inc) work behind it as behind ig_balance_build.  The snapshot is read only: a fetch or a coarsening
 * behind the build sees the bytes it saw before. */

/* the passes ig_debug_balance_snapshot_time reports, in this order */
#define BALSNAP_P_COUNT 0
#define BALSNAP_P_ROWS 1
#define BALSNAP_P_SCATTER 2
#define BALSNAP_P_SORT_SHORT 3
#define BALSNAP_P_SORT_LDS 4
#define BALSNAP_P_SORT_LONG 5
#define BALSNAP_P_GATHER 6
#define BALSNAP_PASSES 7

/* The build up to the rows' fields.  *d_group: the groups on the device (mode != 0), the caller frees it. */
static int balsnap_build_impl(ig_ctx* c, const char* who, int ignore_diags, int mode, const int32_t* group, float* ms, long long scalars[8], int** d_group)
{
    BalBuf& p = c->bal;
    const LiftBuf& l = c->lift;
    const long long U = l.n_units, K = l.n_entries;
    const int Ui = (int)U;
    LiftTimer timer(c, ms, BALSNAP_PASSES);
    DALLOC(p.sc, (size_t)BAL_NS);
    DALLOC(p.total, (size_t)U);
    HIPCK(hipMemsetAsync(p.sc, 0, BAL_NS * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(p.total, 0, (size_t)std::max<long long>(U, 1) * sizeof(unsigned long long), c->stream));
    if (mode != 0) {
        DALLOC(*d_group, (size_t)U);
        if (U > 0) HIPCK(hipMemcpyAsync(*d_group, group, (size_t)U * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    const unsigned long long* s_rowptr = l.rows.rowptr;
    const int* s_col = l.rows.out_col;
    const unsigned long long* s_cnt = l.rows.out_cnt;
    const int* g = *d_group;
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (K == 0 || U < 1) return; /* an empty snapshot: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(K)), block(LIFT_THREADS);
        if (!scatter) hipLaunchKernelGGL((k_balsnap_emit<false>), grid, block, 0, c->stream, s_rowptr, s_col, s_cnt, Ui, K, ignore_diags, mode, g, slots, p.total, ent, n_ent, p.sc);
        else hipLaunchKernelGGL((k_balsnap_emit<true>), grid, block, 0, c->stream, s_rowptr, s_col, s_cnt, Ui, K, ignore_diags, mode, g, slots, p.total, ent, n_ent, p.sc);
    };
    unsigned long long sc[BALSNAP_NS];
    auto check = [&](long long E) {
        for (int k = 0; k < BALSNAP_NS; k++) scalars[k] = (long long)sc[k];
        if (E < 0 || E > 2 * K || (E & 1) || (E > 0 && U < 2)) return fail("%s: %lld entries of %lld snapshot entries over %lld units (device error)", who, E, K, U);
        if (E > 0x7fffffffll) return fail("%s: %lld entries are more than one call can sort (2^31 - 1)", who, E);
        /* the totals: the count pass has summed them (the stream was waited for); every count must convert to a double exactly */
        p.h_total.assign((size_t)U, 0);
        if (U > 0) HIPCK(hipMemcpy(p.h_total.data(), p.total, (size_t)U * sizeof(long long), hipMemcpyDeviceToHost));
        for (long long t : p.h_total)
            if (t < 0 || t >= (1ll << 53)) return fail("%s: the contacts of a unit sum to 2^53 or more (the counts must convert to doubles exactly)", who);
        return 0;
    };
    /* per entry: the word itself, the long rows' scratch and their runs' items (8 bytes each), and an entry of the result (column,
     * count: 12 bytes); the snapshot stays resident beside them */
    const RowsSpec spec = {p.sc, BALSNAP_NS, BALSNAP_ENTRIES, 36, " (the rows of the balancing beside the resident snapshot)", false,
                           {BALSNAP_P_COUNT, BALSNAP_P_ROWS, BALSNAP_P_SCATTER, BALSNAP_P_SORT_SHORT, BALSNAP_P_GATHER}};
    long long E = 0, n_out = 0;
    if (rows_build(c, who, p.rows, Ui, spec, sc, check, emit, timer, p.forms, &E, &n_out)) return -1;
    if (n_out > 0) { /* the sorted words become columns and 64-bit counts; the words go */
        DALLOC(p.rows.out_col, (size_t)n_out);
        DALLOC(p.rows.out_cnt, (size_t)n_out);
        timer.begin();
        hipLaunchKernelGGL(k_balsnap_gather, dim3(lift_blocks(n_out)), dim3(LIFT_THREADS), 0, c->stream, p.rows.ent, n_out, s_cnt, K, p.rows.out_col, p.rows.out_cnt);
        timer.end(BALSNAP_P_GATHER);
    }
    HIPCK(hipStreamSynchronize(c->stream));
    hipFree(p.rows.ent);
    p.rows.ent = nullptr;
    p.level = 1;
    p.n_placed = l.n_placed;
    p.n_units = U;
    p.n_entries = n_out;
    scalars[5] = K;
    scalars[6] = U;
    scalars[7] = n_out;
    return 0;
}

/* group: [n_group] on the host, read at mode != 0 only */
static int balsnap_build(ig_ctx* c, const char* who, int ignore_diags, int mode, const int32_t* group, long long n_group, float* ms, long long scalars[8])
{
    free_bal_buffers(c); /* whatever happens, the result of an earlier build is gone */
    const LiftBuf& l = c->lift;
    if (!l.valid) return fail("%s: no snapshot is built (ig_assembly_contacts_build at level 1, ig_assembly_contacts_build_units, ig_assembly_contacts_coarsen or ig_pairs_pixels_build first)", who);
    if (l.level == 0) return fail("%s: a level 0 snapshot cannot be balanced from (packed words, 32-bit counts): build level 1 or with a unit table", who);
    if (ignore_diags < 1) return fail("%s: ignore_diags must be >= 1: the device holds no diagonal (got %d)", who, ignore_diags);
    if (mode < 0 || mode > 2) return fail("%s: mode is 0 (all), 1 (cis) or 2 (trans), got %d", who, mode);
    if (mode != 0) {
        if (!group) return fail("%s: mode %d needs the group of every unit (NULL group)", who, mode);
        if (n_group != l.n_units) return fail("%s: the groups are for %lld units, the snapshot has %lld", who, n_group, l.n_units);
        for (long long u = 0; u < n_group; u++)
            if (group[u] < 0) return fail("%s: a negative group: unit %lld has %d", who, u, group[u]);
    }
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    if (c->world != 1) return fail("%s: balancing needs all contacts on one handle (this one holds shard %d of %d, and its snapshot that shard's)", who, c->rank, c->world);
    if (l.n_units > 0x7fffffffll) return fail("%s: %lld units are more than 2^31 - 1 (a column is 32 bits)", who, l.n_units);
    if (l.n_entries > 0xffffffffll) return fail("%s: the snapshot has %lld entries, more than a word's index holds (2^32 - 1)", who, l.n_entries);
    int* d_group = nullptr;
    const int rc = balsnap_build_impl(c, who, ignore_diags, mode, group, ms, scalars, &d_group);
    hipStreamSynchronize(c->stream);
    hipFree(d_group);
    bal_free_build(c);
    if (rc) {
        rows_free_result(c->bal.rows); /* (a build that failed behind the sort: its words) */
        bal_release_snapshot(c);
        return rc;
    }
    c->bal.valid = true;
    return 0;
}

extern "C" int ig_balance_build_snapshot(ig_ctx* c, int32_t ignore_diags, int32_t mode, const int32_t* group, int64_t n_group, int64_t* n_units, int64_t* n_entries,
                                         int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_balance_build_snapshot";
    if (!n_units || !n_entries || !scalars) {
        free_bal_buffers(c);
        return fail("%s: NULL output", who);
    }
    long long sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (balsnap_build(c, who, ignore_diags, mode, group, n_group, nullptr, sc)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_units = c->bal.n_units;
    *n_entries = c->bal.n_entries;
    return 0;
}

/* caller CSR data as the handle's snapshot (level 2): what ig_assembly_contacts_rows / _fetch / _coarsen then see */
static int balsnap_load(ig_ctx* c, const int64_t* rowptr, const int32_t* col, const int64_t* count, long long U, long long K)
{
    LiftBuf& l = c->lift;
    DALLOC(l.rows.rowptr, (size_t)U + 1);
    DALLOC(l.rows.out_col, (size_t)K);
    DALLOC(l.rows.out_cnt, (size_t)K);
    HIPCK(hipMemcpyAsync(l.rows.rowptr, rowptr, ((size_t)U + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (K > 0) {
        HIPCK(hipMemcpyAsync(l.rows.out_col, col, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(l.rows.out_cnt, count, (size_t)K * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* ---- tests: the same build over caller CSR data (an upper-triangular map: rowptr [n_rows + 1] from 0, non-decreasing; col >= row,
 * below n_rows, strictly ascending in a row; no negative count), on a bare handle.  The data becomes the handle's snapshot (level 2)
 * and stays it: the one implementation above builds from it. */
extern "C" int ig_debug_balance_snapshot(ig_ctx* c, const int64_t* rowptr, const int32_t* col, const int64_t* count, int64_t n_rows, int32_t ignore_diags, int32_t mode,
                                         const int32_t* group, int64_t n_group, int64_t* n_units, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_balance_snapshot";
    free_bal_buffers(c);
    lift_release_snapshot(c); /* whatever happens, the results of earlier builds are gone */
    if (!n_units || !n_entries || !scalars || !rowptr) return fail("%s: NULL argument", who);
    if (n_rows < 0 || n_rows > 0x7fffffffll) return fail("%s: %lld rows: 0 .. 2^31 - 1", who, (long long)n_rows);
    if (rowptr[0] != 0) return fail("%s: rowptr starts at 0 (got %lld)", who, (long long)rowptr[0]);
    for (int64_t u = 0; u < n_rows; u++)
        if (rowptr[u + 1] < rowptr[u]) return fail("%s: rowptr decreases behind row %lld", who, (long long)u);
    const long long U = n_rows, K = rowptr[n_rows];
    if (K > 0 && (!col || !count)) return fail("%s: NULL argument", who);
    for (long long u = 0; u < U; u++)
        for (long long e = rowptr[u]; e < rowptr[u + 1]; e++) {
            if (col[e] < u || col[e] >= U) return fail("%s: entry %lld of row %lld has column %d: an upper-triangular map has %lld <= column < %lld", who, e, u, col[e], u, U);
            if (e > rowptr[u] && col[e] <= col[e - 1]) return fail("%s: the columns of row %lld do not ascend strictly (entry %lld)", who, u, e);
            if (count[e] < 0) return fail("%s: entry %lld has a negative count", who, e);
            /* (the device sums a unit's total in 64 bits and the host looks at the sum: counts that could wrap it are refused one by one) */
            if (count[e] >= (1ll << 53)) return fail("%s: entry %lld counts 2^53 or more (the counts must convert to doubles exactly)", who, e);
        }
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    LiftBuf& l = c->lift;
    if (balsnap_load(c, rowptr, col, count, U, K)) {
        lift_release_snapshot(c);
        return -1;
    }
    l.level = 2;
    l.n_units = U;
    l.n_entries = K;
    l.n_placed = 0;
    l.valid = true;
    long long sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (balsnap_build(c, who, ignore_diags, mode, group, n_group, nullptr, sc)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_units = c->bal.n_units;
    *n_entries = c->bal.n_entries;
    return 0;
}

/* the build from the resident snapshot (ignore_diags 2, every entry's mode) n times, hipEvents around each pass ->
 * ms_n [n][BALSNAP_PASSES]; the snapshot is read only and the last build's rows stay */
extern "C" int ig_debug_balance_snapshot_time(ig_ctx* c, int32_t n, float* ms_n)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_n) return fail("ig_debug_balance_snapshot_time: bad arguments");
    long long sc[8];
    for (int r = 0; r < n; r++)
        if (balsnap_build(c, "ig_debug_balance_snapshot_time", 2, 0, nullptr, 0, ms_n + (size_t)r * BALSNAP_PASSES, sc)) return -1;
    return 0;
}
