/* ig_host_bal.inc -- part of ig_hip.hip (one translation unit; included there in order): balancing the contact map of the current
 * genome (ig_kernels_bal.cuh; the rule: instagraal_amd/balance.py): the build of the rows (rows_build, ig_host_rows.inc, over the genome
 * view, ig_host_genome.inc), the iteration over them, and the ordered sum on caller data. */

/* the passes ig_debug_balance_time's build reports, in this order */
#define BAL_P_UNITS 0
#define BAL_P_COUNT 1
#define BAL_P_ROWS 2
#define BAL_P_SCATTER 3
#define BAL_P_SORT_SHORT 4
#define BAL_P_SORT_LDS 5
#define BAL_P_SORT_LONG 6
#define BAL_P_REDUCE 7
#define BAL_PASSES 8

#define BAL_SHIP_FORM 1 /* a wave per row: the yardstick.  The packed form has not been shown faster (DESIGN.md 4.19) */
#define BAL_GROUP 8     /* iterations enqueued between two looks at the done flag */
#define BAL_MAX_ITERS (1 << 20)

/* what a build needs and its result does not */
static void bal_free_build(ig_ctx* c)
{
    BalBuf& p = c->bal;
    hipFree(p.key);
    hipFree(p.head);
    hipFree(p.incl);
    hipFree(p.htot);
    hipFree(p.sc);
    hipFree(p.total);
    hipFree(p.unit);
    p.key = p.unit = nullptr;
    p.head = p.incl = p.htot = p.sc = p.total = nullptr;
    rows_free_temp(p.rows);
    rows_free_reserve(p.rows);
}

static void bal_free_run(ig_ctx* c)
{
    BalBuf& p = c->bal;
    hipFree(p.b);
    hipFree(p.marg);
    hipFree(p.dd);
    hipFree(p.var);
    hipFree(p.ctl);
    p.b = p.marg = p.dd = p.var = nullptr;
    p.ctl = nullptr;
}

static void bal_release_snapshot(ig_ctx* c)
{
    BalBuf& p = c->bal;
    rows_free_result(p.rows);
    p.h_total.clear();
    p.valid = false;
    p.n_placed = p.n_units = p.n_entries = 0;
}

/* everything but the settings of ig_debug_balance_form / _group, which belong to the handle */
static void free_bal_buffers(ig_ctx* c)
{
    bal_free_build(c);
    bal_free_run(c);
    bal_release_snapshot(c);
}

/* The build up to the snapshot's fields: the units and every sub-fragment's key, then the rows (rows_build) from k_bal_emit.
 * unit_tab (ig_balance_build_units, ig_host_zoom.inc; else null; level is 1 then): the caller's unit of each of n_positions
 * positions, checked by the caller to be non-decreasing and inside 0 .. n_units_tab - 1. */
static int bal_build_impl(ig_ctx* c, const char* who, int level, int max_side, int ignore_diags, float* ms, long long scalars[8], const int32_t* unit_tab = nullptr,
                          long long n_positions = 0, long long n_units_tab = 0)
{
    BalBuf& p = c->bal;
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    if (c->world != 1) return fail("%s: balancing needs all contacts on one handle (this one holds shard %d of %d)", who, c->rank, c->world);
    int T = 0;
    long long U = 0;
    if (level == 2) {
        GenomeDims d;
        if (genome_view(c, who, max_side, 0, &d)) return -1;
        T = d.T;
        U = d.side;
    } else {
        if (genome_positions(c, who, 0, &T)) return -1;
        U = T;
    }
    if (unit_tab) {
        if (n_positions != T) return fail("%s: the unit table has %lld entries, the genome %d positions", who, n_positions, T);
        U = n_units_tab;
    }
    const int M = c->M;
    LiftTimer timer(c, ms, BAL_PASSES);
    DALLOC(p.key, (size_t)M);
    DALLOC(p.sc, (size_t)BAL_NS);
    HIPCK(hipMemsetAsync(p.sc, 0, BAL_NS * sizeof(unsigned long long), c->stream));
    timer.begin();
    if (unit_tab) {
        DALLOC(p.unit, (size_t)std::max(T, 1));
        if (T > 0) HIPCK(hipMemcpyAsync(p.unit, unit_tab, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    } else if (level == 1 && T > 0) {
        DALLOC(p.head, (size_t)T + 1);
        DALLOC(p.incl, (size_t)T + 1);
        DALLOC(p.htot, (size_t)scan_chunks(T + 1));
        hipLaunchKernelGGL(k_lift_heads, dim3((T + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->sub_tab, c->genome.order, T, p.head);
        scan64_enqueue(c, p.head, p.incl, 0, T, 1, p.htot);
        unsigned long long n_units = 0;
        HIPCK(hipMemcpyAsync(&n_units, p.incl + (T - 1), sizeof(n_units), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        if (n_units < 1 || n_units > (unsigned long long)T) return fail("%s: %llu units over %d positions (inconsistent tables)", who, n_units, T);
        U = (long long)n_units;
    }
    /* (level 2: the view's pixels are the units already; k_lift_keys keeps those inside 0 .. U - 1) */
    if (unit_tab)
        hipLaunchKernelGGL(k_zoom_keys, dim3((M + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->genome.pix, M, T, p.unit, p.key);
    else
        hipLaunchKernelGGL(k_lift_keys, dim3((M + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->genome.pix, M, level == 2 ? (int)U : T,
                           level == 1 && T > 0 ? p.incl : nullptr, p.key);
    timer.end(BAL_P_UNITS);
    const int Ui = (int)U;
    DALLOC(p.total, (size_t)U);
    HIPCK(hipMemsetAsync(p.total, 0, (size_t)U * sizeof(unsigned long long), c->stream));
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (c->Z == 0) return; /* no contacts: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(c->Z)), block(BAL_THREADS);
        if (!scatter) hipLaunchKernelGGL((k_bal_emit<false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, p.key, Ui, ignore_diags, slots, p.total, ent, n_ent, p.sc);
        else hipLaunchKernelGGL((k_bal_emit<true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, p.key, Ui, ignore_diags, slots, p.total, ent, n_ent, p.sc);
    };
    unsigned long long sc[BAL_NS];
    auto check = [&](long long E) {
        for (int k = 0; k < BAL_NS; k++) scalars[k] = (long long)sc[k];
        if (E < 0 || E > 2 * (long long)c->Z || (E & 1) || (E > 0 && U < 2))
            return fail("%s: %lld entries of %lld contacts over %lld units (device error)", who, E, (long long)c->Z, U);
        if (E > 0x7fffffffll) return fail("%s: %lld entries are more than one call can sort (2^31 - 1)", who, E);
        /* the totals: the count pass has summed them (the stream was waited for); every count must convert to a double exactly */
        p.h_total.assign((size_t)U, 0);
        if (U > 0) HIPCK(hipMemcpy(p.h_total.data(), p.total, (size_t)U * sizeof(long long), hipMemcpyDeviceToHost));
        for (long long t : p.h_total)
            if (t < 0 || t >= (1ll << 53)) return fail("%s: the contacts of a unit sum to 2^53 or more (the counts must convert to doubles exactly)", who);
        return 0;
    };
    /* per entry: the word itself, the long rows' scratch and their runs' items (8 bytes each), a bit, and a summed entry of its own
     * (column, count: 12 bytes) */
    const RowsSpec spec = {p.sc, BAL_NS, BAL_ENTRIES, 37, "", true, {BAL_P_COUNT, BAL_P_ROWS, BAL_P_SCATTER, BAL_P_SORT_SHORT, BAL_P_REDUCE}};
    long long E = 0, n_sum = 0;
    if (rows_build(c, who, p.rows, Ui, spec, sc, check, emit, timer, p.forms, &E, &n_sum)) return -1;
    HIPCK(hipStreamSynchronize(c->stream));
    p.level = level;
    p.n_placed = T;
    p.n_units = U;
    p.n_entries = n_sum;
    scalars[5] = T;
    scalars[6] = U;
    scalars[7] = n_sum;
    return 0;
}

static int bal_build(ig_ctx* c, const char* who, int level, int max_side, int ignore_diags, float* ms, long long scalars[8], const int32_t* unit_tab = nullptr,
                     long long n_positions = 0, long long n_units_tab = 0)
{
    free_bal_buffers(c); /* whatever happens, the result of an earlier build is gone */
    if (level < 0 || level > 2) return fail("%s: level is 0 (sub-fragments), 1 (bins) or 2 (the pixels of the contact map), got %d", who, level);
    if (level == 2 && max_side < 1) return fail("%s: max_side must be >= 1 (got %d)", who, max_side);
    if (ignore_diags < 1) return fail("%s: ignore_diags must be >= 1: the device holds no diagonal (got %d)", who, ignore_diags);
    const int rc = bal_build_impl(c, who, level, max_side, ignore_diags, ms, scalars, unit_tab, n_positions, n_units_tab);
    bal_free_build(c);
    if (rc) {
        bal_release_snapshot(c);
        return rc;
    }
    c->bal.valid = true;
    return 0;
}

extern "C" int ig_balance_build(ig_ctx* c, int32_t level, int32_t max_side, int32_t ignore_diags, int64_t* n_units, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!n_units || !n_entries || !scalars) return fail("ig_balance_build: NULL output");
    long long sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (bal_build(c, "ig_balance_build", level, max_side, ignore_diags, nullptr, sc)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_units = c->bal.n_units;
    *n_entries = c->bal.n_entries;
    return 0;
}

/* rowptr: [n_units + 1]; nnz, total: [n_units]; capacity: the words of rowptr */
extern "C" int ig_balance_rows(ig_ctx* c, int64_t* rowptr, int64_t* nnz, int64_t* total, int64_t capacity)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    BalBuf& p = c->bal;
    if (!p.valid) return fail("ig_balance_rows: nothing is built (ig_balance_build first)");
    if (!rowptr || !nnz || !total) return fail("ig_balance_rows: NULL output");
    if (capacity < p.n_units + 1) return fail("ig_balance_rows: the rows need %lld words, the caller's capacity is %lld", p.n_units + 1, (long long)capacity);
    HIPCK(hipMemcpy(rowptr, p.rows.rowptr, ((size_t)p.n_units + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (long long u = 0; u < p.n_units; u++) {
        nnz[u] = rowptr[u + 1] - rowptr[u];
        total[u] = p.h_total[(size_t)u];
    }
    return 0;
}

extern "C" int ig_balance_fetch(ig_ctx* c, int64_t first, int64_t n, int32_t* col, int64_t* count)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    BalBuf& p = c->bal;
    if (!p.valid) return fail("ig_balance_fetch: nothing is built (ig_balance_build first)");
    if (first < 0 || n < 0 || first > p.n_entries || n > p.n_entries - first)
        return fail("ig_balance_fetch: entries %lld .. %lld are out of range (the result has %lld)", (long long)first, (long long)first + (long long)n, p.n_entries);
    if (n == 0) return 0;
    if (!col || !count) return fail("ig_balance_fetch: NULL output");
    HIPCK(hipMemcpy(col, p.rows.out_col + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(count, p.rows.out_cnt + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ig_balance_release(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    free_bal_buffers(c);
    return 0;
}

static inline int bal_form(const ig_ctx* c) { return c->bal.form ? c->bal.form : BAL_SHIP_FORM; }

/* out[row] = the ordered sum of the row (raw: of r.values; otherwise of count * b[col], times b[row]) in the handle's form */
static void bal_enqueue_marginals(ig_ctx* c, const BalRows& r, long long n_rows, long long n_ent, bool raw, const int* done, double* out)
{
    if (n_rows <= 0) return;
    const bool packed = bal_form(c) == 2;
    const long long waves = packed ? (n_rows + 64 / BAL_PACK_LANES - 1) / (64 / BAL_PACK_LANES) : n_rows;
    const dim3 grid((unsigned)((waves + BAL_THREADS / 64 - 1) / (BAL_THREADS / 64))), block(BAL_THREADS);
    if (raw && packed) hipLaunchKernelGGL((k_bal_marginals<true, true>), grid, block, 0, c->stream, r, n_rows, n_ent, done, out);
    else if (raw) hipLaunchKernelGGL((k_bal_marginals<true, false>), grid, block, 0, c->stream, r, n_rows, n_ent, done, out);
    else if (packed) hipLaunchKernelGGL((k_bal_marginals<false, true>), grid, block, 0, c->stream, r, n_rows, n_ent, done, out);
    else hipLaunchKernelGGL((k_bal_marginals<false, false>), grid, block, 0, c->stream, r, n_rows, n_ent, done, out);
}

/* one iteration of the rule behind the done flag: marginals, k and mean, the update, the variance */
static void bal_enqueue_iteration(ig_ctx* c, const BalRows& r, double tol, int max_iters)
{
    BalBuf& p = c->bal;
    const long long U = p.n_units;
    bal_enqueue_marginals(c, r, U, p.n_entries, false, &p.ctl->done, p.marg);
    hipLaunchKernelGGL(k_bal_mean, dim3(1), dim3(BAL_THREADS), 0, c->stream, p.marg, U, p.ctl);
    hipLaunchKernelGGL(k_bal_update, dim3((unsigned)((U + BAL_THREADS - 1) / BAL_THREADS)), dim3(BAL_THREADS), 0, c->stream, p.marg, U, p.ctl, p.b, p.dd);
    hipLaunchKernelGGL(k_bal_var, dim3(1), dim3(64), 0, c->stream, p.dd, U, p.ctl, tol, max_iters, p.var);
}

/* the run's vectors on the device, b = b0 */
static int bal_run_setup(ig_ctx* c, const double* b0, int max_iters, BalRows* r)
{
    BalBuf& p = c->bal;
    const size_t U = (size_t)p.n_units;
    bal_free_run(c);
    DALLOC(p.b, U);
    DALLOC(p.marg, U);
    DALLOC(p.dd, U);
    DALLOC(p.var, (size_t)max_iters);
    DALLOC(p.ctl, 1);
    HIPCK(hipMemcpyAsync(p.b, b0, U * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemsetAsync(p.var, 0, (size_t)max_iters * sizeof(double), c->stream));
    HIPCK(hipMemsetAsync(p.ctl, 0, sizeof(BalCtl), c->stream));
    *r = BalRows{p.rows.rowptr, p.rows.out_col, p.rows.out_cnt, p.b, nullptr};
    return 0;
}

static int bal_run_impl(ig_ctx* c, const char* who, const double* b0, double tol, int max_iters, double* b, double* marg_final, double* variance, int32_t* n_iters,
                        int32_t* converged)
{
    BalBuf& p = c->bal;
    const size_t U = (size_t)p.n_units;
    bool any = false;
    for (size_t u = 0; u < U && !any; u++) any = b0[u] != 0.0;
    *n_iters = *converged = 0;
    for (int k = 0; k < max_iters; k++) variance[k] = 0.0;
    if (p.n_entries == 0 || !any) { /* every marginal is zero: the rule stops in front of its first iteration; nothing is launched */
        for (size_t u = 0; u < U; u++) b[u] = b0[u], marg_final[u] = 0.0;
        return 0;
    }
    BalRows r;
    if (bal_run_setup(c, b0, max_iters, &r)) return -1;
    const int group = p.group > 0 ? p.group : BAL_GROUP;
    BalCtl ctl{};
    for (int queued = 0; queued < max_iters && !ctl.done;) {
        const int n = std::min(group, max_iters - queued);
        for (int k = 0; k < n; k++) bal_enqueue_iteration(c, r, tol, max_iters);
        queued += n;
        HIPCK(hipMemcpyAsync(&ctl, p.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    if (ctl.n_iters < 0 || ctl.n_iters > max_iters) return fail("%s: %d iterations of at most %d (device error)", who, ctl.n_iters, max_iters);
    bal_enqueue_marginals(c, r, p.n_units, p.n_entries, false, nullptr, p.marg); /* one more, from the final b */
    HIPCK(hipMemcpyAsync(b, p.b, U * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(marg_final, p.marg, U * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (ctl.n_iters > 0) HIPCK(hipMemcpyAsync(variance, p.var, (size_t)ctl.n_iters * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    *n_iters = ctl.n_iters;
    *converged = ctl.converged;
    return 0;
}

/* b0, b, marg_final: [n_units]; variance: [max_iters], zero beyond n_iters */
extern "C" int ig_balance_run(ig_ctx* c, const double* b0, double tol, int32_t max_iters, double* b, double* marg_final, double* variance, int32_t* n_iters,
                              int32_t* converged)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->bal.valid) return fail("ig_balance_run: nothing is built (ig_balance_build first)");
    if (!(tol >= 0.0)) return fail("ig_balance_run: tol must be >= 0 (got %g)", tol);
    if (max_iters < 1 || max_iters > BAL_MAX_ITERS) return fail("ig_balance_run: 1 <= max_iters <= %d (got %d)", BAL_MAX_ITERS, max_iters);
    if (!b0 || !b || !marg_final || !variance || !n_iters || !converged) return fail("ig_balance_run: NULL argument");
    if (c->nuis_in_flight || c->chain_busy) return fail("ig_balance_run: a nuisance step or a chain is in flight");
    const int rc = bal_run_impl(c, "ig_balance_run", b0, tol, max_iters, b, marg_final, variance, n_iters, converged);
    bal_free_run(c);
    return rc;
}

extern "C" int ig_debug_balance_form(ig_ctx* c, int32_t form)
{
    IG_JOIN(c);
    if (form < 0 || form > 2) return fail("ig_debug_balance_form: 0 (the default), 1 (a wave per row) or 2 (packed: short rows share a wave), got %d", form);
    c->bal.form = form;
    return 0;
}

extern "C" int ig_debug_balance_group(ig_ctx* c, int32_t group)
{
    IG_JOIN(c);
    if (group < 0) return fail("ig_debug_balance_group: 0 (the default) or the iterations per look at the done flag (got %d)", group);
    c->bal.group = group;
    return 0;
}

static int debug_lane_sums_impl(ig_ctx* c, const double* values, const int64_t* rowptr, long long n_rows, long long n_val, double* out, double*& d_val,
                                unsigned long long*& d_ptr, double*& d_out)
{
    DALLOC(d_val, (size_t)n_val);
    DALLOC(d_ptr, (size_t)n_rows + 1);
    DALLOC(d_out, (size_t)n_rows);
    if (n_val > 0) HIPCK(hipMemcpyAsync(d_val, values, (size_t)n_val * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d_ptr, rowptr, ((size_t)n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    const BalRows r = {d_ptr, nullptr, nullptr, nullptr, d_val};
    bal_enqueue_marginals(c, r, n_rows, n_val, true, nullptr, d_out);
    HIPCK(hipMemcpyAsync(out, d_out, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* the ordered sum over caller data, in the handle's form: values [rowptr[n_rows]], rowptr [n_rows + 1] from 0 and non-decreasing,
 * out [n_rows].  Reads nothing uploaded to the handle: a created handle is enough. */
extern "C" int ig_debug_lane_sums(ig_ctx* c, const double* values, const int64_t* rowptr, int64_t n_rows, double* out)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!rowptr || !out) return fail("ig_debug_lane_sums: NULL argument");
    if (n_rows < 1 || n_rows > 0x7fffffffll) return fail("ig_debug_lane_sums: 1 <= n_rows < 2^31 (got %lld)", (long long)n_rows);
    if (rowptr[0] != 0) return fail("ig_debug_lane_sums: rowptr starts at 0");
    for (int64_t k = 0; k < n_rows; k++)
        if (rowptr[k + 1] < rowptr[k]) return fail("ig_debug_lane_sums: rowptr decreases at row %lld", (long long)k);
    const long long n_val = rowptr[n_rows];
    if (n_val > 0 && !values) return fail("ig_debug_lane_sums: NULL argument");
    if (c->nuis_in_flight || c->chain_busy) return fail("ig_debug_lane_sums: a nuisance step or a chain is in flight");
    double *d_val = nullptr, *d_out = nullptr;
    unsigned long long* d_ptr = nullptr;
    const int rc = debug_lane_sums_impl(c, values, rowptr, n_rows, n_val, out, d_val, d_ptr, d_out);
    hipFree(d_val);
    hipFree(d_ptr);
    hipFree(d_out);
    return rc;
}

/* what = 0: the marginals kernel alone; 1: one whole iteration (marginals, mean, update, variance), n times each from b = 1 with the
 * done flag never set (tol = 0) -> ms_n [n], event-timed; the rows must be built.  The run's vectors are freed behind it. */
extern "C" int ig_debug_balance_time(ig_ctx* c, int32_t what, int32_t n, float* ms_n)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    BalBuf& p = c->bal;
    if (n < 1 || !ms_n || what < 0 || what > 1) return fail("ig_debug_balance_time: bad arguments");
    if (!p.valid) return fail("ig_debug_balance_time: nothing is built (ig_balance_build first)");
    if (p.n_units < 1) return fail("ig_debug_balance_time: no unit");
    const std::vector<double> ones((size_t)p.n_units, 1.0);
    BalRows r;
    int rc = bal_run_setup(c, ones.data(), n, &r);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail("ig_debug_balance_time: the run's vectors could not be set up");
    if (!rc)
        rc = time_repeats(c, "ig_debug_balance_time", n, ms_n, [&] {
            if (what == 0) bal_enqueue_marginals(c, r, p.n_units, p.n_entries, false, nullptr, p.marg);
            else bal_enqueue_iteration(c, r, 0.0, n);
            return 0;
        });
    bal_free_run(c);
    return rc;
}

extern "C" int ig_debug_balance_build_time(ig_ctx* c, int32_t level, int32_t max_side, int32_t ignore_diags, int32_t n, float* ms_n)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_n) return fail("ig_debug_balance_build_time: bad arguments");
    long long sc[8];
    for (int r = 0; r < n; r++)
        if (bal_build(c, "ig_debug_balance_build_time", level, max_side, ignore_diags, ms_n + (size_t)r * BAL_PASSES, sc)) return -1;
    return 0;
}
