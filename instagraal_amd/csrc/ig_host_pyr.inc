/* ig_host_pyr.inc -- part of ig_hip.hip (one translation unit; included there in order): the contact levels of the pyramid
 * (ig_kernels_pyr.cuh; the rule: instagraal_amd/pyramid_levels.py; DESIGN.md 4.28).  A session on a created handle with nothing
 * uploaded: the level-0 list in pieces (ig_pyr_begin), its level through the row builder (ig_pyr_matrix), the degrees of the filter
 * (ig_pyr_degrees), the next level from the current one, which never leaves the device (ig_pyr_remap: two RowBufs swap roles), and
 * the current level as data3's three rows (ig_pyr_rows, ig_pyr_fetch). */

/* PyrBuf.sc, in 64-bit words */
#define PYR_SC_EMIT 0
#define PYR_SC_CANON PYR_NS
#define PYR_SC_LARGEST (PYR_NS + 1)
#define PYR_SC_BAD (PYR_NS + 2)
#define PYR_SC_WORDS (PYR_NS + 3)
#define PYR_PIECE (1ll << 22) /* entries of the list that go to the device at a time */

static void pyr_free_list(PyrBuf& p)
{
    hipFree(p.a);
    hipFree(p.b);
    hipFree(p.cnt);
    p.a = p.b = p.cnt = nullptr;
    p.n0 = 0;
}

static void free_pyr_buffers(ig_ctx* c)
{
    PyrBuf& p = c->pyr;
    pyr_free_list(p);
    hipFree(p.lut);
    hipFree(p.deg);
    for (int k = 0; k < 3; k++) hipFree(p.out[k]);
    hipFree(p.sc);
    rows_free(p.rows[0]);
    rows_free(p.rows[1]);
    const long long piece = p.piece; /* (the handle's setting, not the session's) */
    p = PyrBuf{};
    p.piece = piece;
}

static int pyr_usable(ig_ctx* c, const char* who)
{
    if (!c->pyr.live) return fail("%s: no session (ig_pyr_begin first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    return 0;
}

/* entries per upload piece (0: the default, PYR_PIECE): for tests of the upload in pieces */
extern "C" int ig_debug_pyr_piece(ig_ctx* c, int64_t entries)
{
    if (entries < 0) return fail("ig_debug_pyr_piece: %lld entries", (long long)entries);
    c->pyr.piece = entries;
    return 0;
}

/* The level-0 list of n entries over n_frags fragments, in file order: a, b 0-based ids, count.  *is_canonical: every a <= b and the
 * pairs strictly ascending, i.e. the list is its own level. */
extern "C" int ig_pyr_begin(ig_ctx* c, int32_t n_frags, const int32_t* a, const int32_t* b, const int64_t* count, int64_t n, int32_t* is_canonical)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pyr_begin";
    PyrBuf& p = c->pyr;
    if (p.live) return fail("%s: a session is open (ig_pyr_end first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    if (n_frags < 1 || n < 0 || n > 0x7fffffffll) return fail("%s: bad sizes (%d fragments, %lld entries)", who, n_frags, (long long)n);
    if (!is_canonical || (n > 0 && (!a || !b || !count))) return fail("%s: NULL argument", who);
    for (long long k = 0; k < n; k++) { /* the refusals, before anything is allocated */
        if (a[k] < 0 || a[k] >= n_frags || b[k] < 0 || b[k] >= n_frags)
            return fail("%s: entry %lld is (%d, %d): ids are 0 .. %d", who, k, a[k], b[k], n_frags - 1);
        if (count[k] < 0) return fail("%s: entry %lld has the count %lld", who, k, (long long)count[k]);
        if ((unsigned long long)count[k] >= PYR_LIMIT) return fail("%s: entry %lld has the count %lld: 2^31 or more, so is the sum of its pixel", who, k, (long long)count[k]);
    }
    if (rows_memory_guard(who, n, 3 * sizeof(int), n_frags, " (the level-0 list)")) return -1;
    const long long piece = p.piece > 0 ? p.piece : PYR_PIECE;
    std::vector<int> staged((size_t)std::min<long long>(piece, std::max<long long>(n, 1)));
    unsigned long long h_canon = 0;
    const int rc = [&]() -> int {
        DALLOC(p.a, (size_t)n);
        DALLOC(p.b, (size_t)n);
        DALLOC(p.cnt, (size_t)n);
        DALLOC(p.sc, (size_t)PYR_SC_WORDS);
        HIPCK(hipMemsetAsync(p.sc, 0, PYR_SC_WORDS * sizeof(unsigned long long), c->stream));
        for (long long o = 0; o < n; o += piece) {
            const long long m = std::min<long long>(piece, n - o);
            for (long long k = 0; k < m; k++) staged[(size_t)k] = (int)count[o + k];
            HIPCK(hipMemcpyAsync(p.a + o, a + o, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCK(hipMemcpyAsync(p.b + o, b + o, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCK(hipMemcpyAsync(p.cnt + o, staged.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCK(hipStreamSynchronize(c->stream)); /* (the staging array is the next piece's) */
        }
        if (n > 0)
            hipLaunchKernelGGL(k_pyr_canon, dim3(lift_blocks(n)), dim3(PYR_THREADS), 0, c->stream, (const int*)p.a, (const int*)p.b, (long long)n, p.sc + PYR_SC_CANON);
        HIPCK(hipMemcpyAsync(&h_canon, p.sc + PYR_SC_CANON, sizeof(h_canon), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        free_pyr_buffers(c);
        return rc;
    }
    if (h_canon > (unsigned long long)n) {
        free_pyr_buffers(c);
        return fail("%s: %llu of %lld entries out of order (device error)", who, h_canon, (long long)n);
    }
    p.live = true;
    p.have_level = false;
    p.n_frags = n_frags, p.n0 = n, p.n_out = 0, p.cur = 0;
    p.canonical = h_canon == 0 ? 1 : 0;
    *is_canonical = p.canonical;
    return 0;
}

/* One level from the current one: through d_lut (null: the ids as they are) into U_new fragments, the first `skip` entries of the
 * source passed over.  The source is rows[cur], or the uploaded list while no level has been made; the result is built in the
 * other RowBuf and, once nothing can refuse it any more, the two swap roles.  A refusal leaves the current level as it was. */
static int pyr_build(ig_ctx* c, const char* who, const int* d_lut, int U_new, long long skip, long long* n_pixels, long long sc_out[8], float* ms)
{
    PyrBuf& p = c->pyr;
    RowBuf &src = p.rows[p.cur], &dst = p.rows[p.cur ^ 1];
    const bool raw = !p.have_level;
    const long long n_in = raw ? p.n0 : p.n_out;
    const int U_old = p.n_frags;
    rows_free_temp(dst);
    rows_free_result(dst);
    long long n_out = 0;
    unsigned long long h_sc[PYR_NS] = {0, 0, 0, 0}, h_top[2] = {0, ~0ull};
    const int rc = [&]() -> int {
        unsigned long long* d_sc = p.sc + PYR_SC_EMIT;
        HIPCK(hipMemsetAsync(p.sc, 0, (PYR_SC_WORDS - 1) * sizeof(unsigned long long), c->stream));
        HIPCK(hipMemsetAsync(p.sc + PYR_SC_BAD, 0xff, sizeof(unsigned long long), c->stream));
        auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
            if (n_in == 0) return; /* an empty source: nothing to launch, the rows stay empty */
            const dim3 grid(lift_blocks(n_in)), block(PYR_THREADS);
#define PYR_EMIT(S, R)                                                                                                                                             \
    hipLaunchKernelGGL((k_pyr_emit<S, R>), grid, block, 0, c->stream, (const int*)p.a, (const int*)p.b, (const int*)p.cnt, (const unsigned long long*)src.rowptr, \
                       (const int*)src.out_col, (const unsigned long long*)src.out_cnt, n_in, U_old, d_lut, U_new, skip, slots, ent, n_ent, d_sc)
            if (!scatter && raw) PYR_EMIT(false, true);
            else if (!scatter) PYR_EMIT(false, false);
            else if (raw) PYR_EMIT(true, true);
            else PYR_EMIT(true, false);
#undef PYR_EMIT
        };
        auto check = [&](long long E) {
            const unsigned long long want_skip = (unsigned long long)std::min<long long>(skip, n_in);
            if (h_sc[PYR_IN] != (unsigned long long)n_in || h_sc[PYR_SKIPPED] != want_skip || h_sc[PYR_SKIPPED] + h_sc[PYR_DROPPED] + h_sc[PYR_KEPT] != (unsigned long long)n_in ||
                (unsigned long long)E != h_sc[PYR_KEPT] || (!d_lut && h_sc[PYR_DROPPED] != 0))
                return fail("%s: %llu entries counted of %lld, %llu skipped, %llu dropped, %llu kept (device error)", who, h_sc[PYR_IN], n_in, h_sc[PYR_SKIPPED],
                            h_sc[PYR_DROPPED], h_sc[PYR_KEPT]);
            return 0;
        };
        /* per entry: the word, the long rows' scratch and their runs' items (8 bytes each), a bit, a summed entry (12 bytes) */
        const RowsSpec spec = {d_sc, PYR_NS, PYR_KEPT, 37, " (the level's temporaries)", true, {LIFT_P_COUNT, LIFT_P_SCAN, LIFT_P_SCATTER, LIFT_P_SORT_SHORT, LIFT_P_REDUCE}};
        LiftTimer timer(c, ms, LIFT_PASSES);
        long long E = 0;
        if (rows_build(c, who, dst, U_new, spec, h_sc, check, emit, timer, p.forms, &E, &n_out)) return -1;
        if (n_out > 0) {
            hipLaunchKernelGGL(k_pyr_largest, dim3(lift_blocks(n_out)), dim3(PYR_THREADS), 0, c->stream, (const unsigned long long*)dst.out_cnt, n_out, p.sc + PYR_SC_LARGEST,
                               p.sc + PYR_SC_BAD);
            HIPCK(hipMemcpyAsync(h_top, p.sc + PYR_SC_LARGEST, sizeof(h_top), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCK(hipStreamSynchronize(c->stream));
        if (h_top[1] != ~0ull) { /* the refusal of the rule: name the pixel */
            const unsigned long long g = h_top[1];
            if (g >= (unsigned long long)n_out) return fail("%s: the pixel %llu of %lld (device error)", who, g, n_out);
            std::vector<unsigned long long> rowptr((size_t)U_new + 1);
            int col = 0;
            unsigned long long sum = 0;
            HIPCK(hipMemcpy(rowptr.data(), dst.rowptr, rowptr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            HIPCK(hipMemcpy(&col, dst.out_col + g, sizeof(col), hipMemcpyDeviceToHost));
            HIPCK(hipMemcpy(&sum, dst.out_cnt + g, sizeof(sum), hipMemcpyDeviceToHost));
            const long long row = (long long)(std::upper_bound(rowptr.begin(), rowptr.end(), g) - rowptr.begin()) - 1;
            return fail("%s: the sum of the pixel (%lld, %d) is %llu: 2^31 or more does not fit the level's int32", who, row, col, sum);
        }
        return 0;
    }();
    hipStreamSynchronize(c->stream);
    rows_free_temp(dst);
    if (rc) {
        rows_free_result(dst);
        return rc;
    }
    if (raw) pyr_free_list(p);
    else rows_free_result(src);
    p.cur ^= 1;
    p.have_level = true;
    p.n_frags = U_new;
    p.n_out = n_out;
    const long long sc[8] = {n_in, (long long)h_sc[PYR_SKIPPED], (long long)h_sc[PYR_DROPPED], (long long)h_sc[PYR_KEPT], n_out, (long long)h_top[0], 0, 0};
    if (sc_out)
        for (int k = 0; k < 8; k++) sc_out[k] = sc[k];
    *n_pixels = n_out;
    return 0;
}

/* The level of the uploaded list: the upper-triangular sum over (min, max), rows and columns ascending; it becomes the current level.
 * With a level already made, its size.  ms (may be null): LIFT_PASSES words. */
extern "C" int ig_pyr_matrix(ig_ctx* c, int64_t* n_pixels, float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pyr_matrix";
    if (pyr_usable(c, who)) return -1;
    if (!n_pixels) return fail("%s: NULL output", who);
    PyrBuf& p = c->pyr;
    if (p.have_level) {
        if (ms)
            for (int k = 0; k < LIFT_PASSES; k++) ms[k] = 0.0f;
        *n_pixels = p.n_out;
        return 0;
    }
    long long n = 0;
    if (pyr_build(c, who, nullptr, p.n_frags, 0, &n, nullptr, ms)) return -1;
    *n_pixels = n;
    return 0;
}

/* deg[n_frags] of the current level: the partners of every fragment; a stored zero is none, a diagonal entry counts once */
extern "C" int ig_pyr_degrees(ig_ctx* c, int32_t* deg)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pyr_degrees";
    if (pyr_usable(c, who)) return -1;
    PyrBuf& p = c->pyr;
    if (!p.have_level) return fail("%s: no level is made of the list (ig_pyr_matrix first)", who);
    if (p.n_frags == 0) return 0;
    if (!deg) return fail("%s: NULL output", who);
    const RowBuf& r = p.rows[p.cur];
    if (p.n_frags > p.deg_cap) {
        hipFree(p.deg);
        p.deg = nullptr, p.deg_cap = 0;
        DALLOC(p.deg, (size_t)p.n_frags);
        p.deg_cap = p.n_frags;
    }
    HIPCK(hipMemsetAsync(p.deg, 0, (size_t)p.n_frags * sizeof(unsigned), c->stream));
    if (p.n_out > 0)
        hipLaunchKernelGGL(k_pyr_degrees, dim3(lift_blocks(p.n_out)), dim3(PYR_THREADS), 0, c->stream, (const unsigned long long*)r.rowptr, p.n_frags, (const int*)r.out_col,
                           (const unsigned long long*)r.out_cnt, p.n_out, p.deg);
    HIPCK(hipMemcpyAsync(deg, p.deg, (size_t)p.n_frags * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* The next level from the current one: lut[n_old] (n_old: the fragments of the current level) holds the new id of every fragment,
 * ascending wherever it is not -1, below n_new; skip_first: the first entry of the current level (of the uploaded list: in file
 * order) is lost (quirk Q-P1 of the binning).  scalars: {entries_in, skipped, dropped_by_lut, entries_kept, pixels, largest_sum, 0,
 * 0}.  ms (may be null): LIFT_PASSES words. */
extern "C" int ig_pyr_remap(ig_ctx* c, const int32_t* lut, int32_t n_old, int32_t n_new, int32_t skip_first, int64_t* n_pixels, int64_t scalars[8], float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pyr_remap";
    if (pyr_usable(c, who)) return -1;
    PyrBuf& p = c->pyr;
    if (!n_pixels || !scalars) return fail("%s: NULL output", who);
    if (n_old != p.n_frags) return fail("%s: the table has %d entries, the current level %d fragments", who, n_old, p.n_frags);
    if (n_new < 0 || n_new > n_old) return fail("%s: %d new fragments of %d", who, n_new, n_old);
    if (n_old > 0 && !lut) return fail("%s: NULL argument", who);
    if (skip_first != 0 && skip_first != 1) return fail("%s: skip_first is 0 or 1 (got %d)", who, skip_first);
    int last = 0;
    for (int k = 0; k < n_old; k++) {
        if (lut[k] == -1) continue;
        if (lut[k] < last || lut[k] >= n_new) return fail("%s: the table maps fragment %d to %d: -1, or ascending from %d and below %d", who, k, lut[k], last, n_new);
        last = lut[k];
    }
    if (n_old > p.lut_cap) {
        hipFree(p.lut);
        p.lut = nullptr, p.lut_cap = 0;
        DALLOC(p.lut, (size_t)n_old);
        p.lut_cap = n_old;
    }
    if (n_old > 0) HIPCK(hipMemcpyAsync(p.lut, lut, (size_t)n_old * sizeof(int), hipMemcpyHostToDevice, c->stream));
    long long n = 0, sc[8];
    if (pyr_build(c, who, p.lut, n_new, skip_first, &n, sc, ms)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_pixels = n;
    return 0;
}

/* rowptr[n_frags + 1] of the current level (n_rowptr: the caller's capacity) */
extern "C" int ig_pyr_rows(ig_ctx* c, int64_t* rowptr, int64_t n_rowptr)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pyr_rows";
    if (pyr_usable(c, who)) return -1;
    PyrBuf& p = c->pyr;
    if (!p.have_level) return fail("%s: no level is made of the list (ig_pyr_matrix first)", who);
    if (!rowptr || n_rowptr < (long long)p.n_frags + 1) return fail("%s: the result has %lld row words, the caller's capacity is %lld", who, (long long)p.n_frags + 1, (long long)n_rowptr);
    HIPCK(hipMemcpy(rowptr, p.rows[p.cur].rowptr, ((size_t)p.n_frags + 1) * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

/* the entries first .. first + n - 1 of the current level as data3's three rows: row, column, count */
extern "C" int ig_pyr_fetch(ig_ctx* c, int64_t first, int64_t n, int32_t* row, int32_t* col, int32_t* count)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pyr_fetch";
    if (pyr_usable(c, who)) return -1;
    PyrBuf& p = c->pyr;
    if (!p.have_level) return fail("%s: no level is made of the list (ig_pyr_matrix first)", who);
    if (first < 0 || n < 0 || first > p.n_out || n > p.n_out - first) return fail("%s: entries %lld .. %lld of %lld", who, (long long)first, (long long)(first + n), p.n_out);
    if (n > 0 && (!row || !col || !count)) return fail("%s: NULL output", who);
    if (n == 0) return 0;
    if (n > p.out_cap) {
        for (int k = 0; k < 3; k++) hipFree(p.out[k]), p.out[k] = nullptr;
        p.out_cap = 0;
        for (int k = 0; k < 3; k++) DALLOC(p.out[k], (size_t)n);
        p.out_cap = n;
    }
    const RowBuf& r = p.rows[p.cur];
    hipLaunchKernelGGL(k_pyr_expand, dim3(lift_blocks(n)), dim3(PYR_THREADS), 0, c->stream, (const unsigned long long*)r.rowptr, p.n_frags, (const int*)r.out_col,
                       (const unsigned long long*)r.out_cnt, (long long)first, (long long)n, p.out[0], p.out[1], p.out[2]);
    int32_t* host[3] = {row, col, count};
    for (int k = 0; k < 3; k++) HIPCK(hipMemcpyAsync(host[k], p.out[k], (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ig_pyr_end(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->pyr.live) return fail("ig_pyr_end: no session (ig_pyr_begin first)");
    HIPCK(hipStreamSynchronize(c->stream));
    free_pyr_buffers(c);
    return 0;
}
