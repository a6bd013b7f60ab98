/* ig_host_lift.inc -- part of ig_hip.hip (one translation unit; included there in order): the contacts in the coordinates of the
 * current genome (ig_kernels_lift.cuh; the rule: instagraal_amd/assembly_contacts.py): the units, the emit step and the snapshot; the
 * rows are built by rows_build (ig_host_rows.inc) over the genome view (ig_host_genome.inc). */

/* the passes ig_debug_assembly_contacts_time reports, in this order */
#define LIFT_P_COUNT 0
#define LIFT_P_SCAN 1
#define LIFT_P_SCATTER 2
#define LIFT_P_SORT_SHORT 3
#define LIFT_P_SORT_LDS 4
#define LIFT_P_SORT_LONG 5
#define LIFT_P_REDUCE 6
#define LIFT_PASSES 7

/* the built result; the buffers kept from call to call stay */
static void lift_release_snapshot(ig_ctx* c)
{
    LiftBuf& l = c->lift;
    rows_free_result(l.rows);
    l.valid = false;
    l.n_units = l.n_entries = 0;
    l.contacts_kept = l.unplaced[0] = l.unplaced[1] = 0;
}

/* everything but the settings of ig_debug_assembly_contacts_limits / _combine, which belong to the handle */
static void free_lift_buffers(ig_ctx* c)
{
    LiftBuf& l = c->lift;
    rows_free(l.rows);
    hipFree(l.key);
    hipFree(l.head);
    hipFree(l.incl);
    hipFree(l.htot);
    hipFree(l.sc);
    hipFree(l.unit);
    const int short_max = l.short_max, lds_max = l.lds_max;
    const bool no_combine = l.no_combine;
    l = LiftBuf{};
    l.short_max = short_max;
    l.lds_max = lds_max;
    l.no_combine = no_combine;
}

/* The build, up to the snapshot's fields: the units and every sub-fragment's key, then the rows (rows_build) from k_lift_pass.  The
 * caller frees what it leaves behind (rows_free_temp, l.unit) and, on an error, the half-built snapshot.
 * unit_tab (level 2, ig_host_zoom.inc; else null): the caller's unit of each of n_positions positions, checked by the caller to be
 * non-decreasing and inside 0 .. n_units_tab - 1; the rows are summed as at level 1. */
static int lift_build_impl(ig_ctx* c, const char* who, int level, float* ms, const int32_t* unit_tab = nullptr, long long n_positions = 0, long long n_units_tab = 0)
{
    LiftBuf& l = c->lift;
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    int T = 0;
    if (genome_positions(c, who, 0, &T)) return -1;
    const int M = c->M;
    if (l.M != M) {
        free_lift_buffers(c);
        DALLOC(l.key, (size_t)M);
        DALLOC(l.head, (size_t)M + 1);
        DALLOC(l.incl, (size_t)M + 1);
        DALLOC(l.htot, (size_t)scan_chunks(M + 1));
        DALLOC(l.sc, (size_t)LIFT_NS);
        if (rows_reserve(l.rows, M)) return -1;
        l.M = M;
    }
    if (unit_tab && n_positions != T) return fail("%s: the unit table has %lld entries, the genome %d positions", who, n_positions, T);
    LiftTimer timer(c, ms, LIFT_PASSES);
    /* the units */
    long long U = unit_tab ? n_units_tab : T;
    if (level == 1 && T > 0) {
        hipLaunchKernelGGL(k_lift_heads, dim3((T + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->sub_tab, c->genome.order, T, l.head);
        scan64_enqueue(c, l.head, l.incl, 0, T, 1, l.htot);
        unsigned long long n_units = 0;
        HIPCK(hipMemcpyAsync(&n_units, l.incl + (T - 1), sizeof(n_units), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        if (n_units < 1 || n_units > (unsigned long long)T) return fail("%s: %llu units over %d positions (inconsistent tables)", who, n_units, T);
        U = (long long)n_units;
    }
    if (unit_tab) {
        hipFree(l.unit);
        l.unit = nullptr;
        DALLOC(l.unit, (size_t)std::max(T, 1));
        if (T > 0) HIPCK(hipMemcpyAsync(l.unit, unit_tab, (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_zoom_keys, dim3((M + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->genome.pix, M, T, l.unit, l.key);
    } else
        hipLaunchKernelGGL(k_lift_keys, dim3((M + LIFT_THREADS - 1) / LIFT_THREADS), dim3(LIFT_THREADS), 0, c->stream, c->genome.pix, M, T, level == 1 ? l.incl : nullptr,
                           l.key);
    const int Ui = (int)U;
    HIPCK(hipMemsetAsync(l.sc, 0, LIFT_NS * sizeof(unsigned long long), c->stream));
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (c->Z == 0) return; /* no contacts: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(c->Z)), block(LIFT_THREADS);
        if (!scatter && l.no_combine)
            hipLaunchKernelGGL((k_lift_pass<false, false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, slots, ent, n_ent, l.sc, c->rank, c->world);
        else if (!scatter)
            hipLaunchKernelGGL((k_lift_pass<false, true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, slots, ent, n_ent, l.sc, c->rank, c->world);
        else if (l.no_combine)
            hipLaunchKernelGGL((k_lift_pass<true, false>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, slots, ent, n_ent, l.sc, c->rank, c->world);
        else
            hipLaunchKernelGGL((k_lift_pass<true, true>), grid, block, 0, c->stream, c->crow, c->cc, c->Z, l.key, Ui, slots, ent, n_ent, l.sc, c->rank, c->world);
    };
    auto check = [&](long long K) { return K < 0 || K > c->Z ? fail("%s: %lld entries kept of %lld (device error)", who, K, (long long)c->Z) : 0; };
    const RowsSpec spec = {l.sc, LIFT_NS, LIFT_ENTRIES_KEPT, 0, "", level != 0, {LIFT_P_COUNT, LIFT_P_SCAN, LIFT_P_SCATTER, LIFT_P_SORT_SHORT, LIFT_P_REDUCE}};
    unsigned long long sc[LIFT_NS];
    long long K = 0, n_out = 0;
    if (rows_build(c, who, l.rows, Ui, spec, sc, check, emit, timer, l.forms, &K, &n_out)) return -1;
    HIPCK(hipStreamSynchronize(c->stream));
    l.level = level;
    l.n_units = U;
    l.n_entries = n_out;
    l.n_placed = T;
    return 0;
}

/* scalars: the eight words of assembly_contacts.SCALARS */
static int lift_build(ig_ctx* c, const char* who, int level, float* ms, long long scalars[8], const int32_t* unit_tab = nullptr, long long n_positions = 0,
                      long long n_units_tab = 0)
{
    lift_release_snapshot(c); /* whatever happens, the result of an earlier build is gone */
    if (unit_tab ? level != 2 : level != 0 && level != 1) return fail("%s: level is 0 (sub-fragments) or 1 (bins), got %d", who, level);
    const int rc = lift_build_impl(c, who, level, ms, unit_tab, n_positions, n_units_tab);
    rows_free_temp(c->lift.rows);
    hipFree(c->lift.unit);
    c->lift.unit = nullptr;
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
    l.contacts_kept = scalars[LIFT_CONTACTS_KEPT];
    l.unplaced[0] = scalars[LIFT_ENTRIES_UNPLACED];
    l.unplaced[1] = scalars[LIFT_CONTACTS_UNPLACED];
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
    HIPCK(hipMemcpy(rowptr, l.rows.rowptr, ((size_t)l.n_units + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
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
    if (l.level != 0) { /* reduced: the bins, a caller's units, a coarsening */
        HIPCK(hipMemcpy(col, l.rows.out_col + first, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(count, l.rows.out_cnt + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        return 0;
    }
    const int64_t piece = 1 << 22; /* the packed words come through a staging buffer of 32 MiB */
    std::vector<unsigned long long> stage((size_t)std::min(n, piece));
    for (int64_t o = 0; o < n; o += piece) {
        const int64_t m = std::min(piece, n - o);
        HIPCK(hipMemcpy(stage.data(), l.rows.ent + first + o, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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
        std::vector<long long> rows((size_t)l.n_units + 1);
        HIPCK(hipMemcpy(rows.data(), l.rows.rowptr, rows.size() * sizeof(long long), hipMemcpyDeviceToHost));
        unsigned long long s = weighted_checksum(rows.data(), rows.size()), place = rows.size() + 1; /* behind the rows: column, count, column, ... */
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
 * Nothing but the genome view (genome_view) reads `activ`. */
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
