/* ig_host_pairs.inc -- part of ig_hip.hip (one translation unit; included there in order): read pairs lifted onto the current genome
 * (ig_kernels_pairs.cuh; the rule: instagraal_amd/pairs_lift.py; DESIGN.md 4.25): the session (source table, store, staging), the
 * lift of a chunk, the pixels through the row builder (rows_build, ig_host_rows.inc) into the assembly-contacts snapshot
 * (ig_host_lift.inc: ig_assembly_contacts_rows / _fetch / _coarsen / _release serve it unchanged), and the distance histogram. */

/* PairsBuf.sc, in 64-bit words */
#define PAIRS_SC_CURSOR 0
#define PAIRS_SC_LIFT 1
#define PAIRS_SC_EMIT (PAIRS_SC_LIFT + PAIRS_NS)
#define PAIRS_SC_WORDS (PAIRS_SC_EMIT + 2)
#define PAIRS_PIECE (1ll << 22)         /* pairs of a chunk that go through the staging arrays at a time */
#define PAIRS_MAX_STORE 0x7fffffffll    /* pairs the store holds at the most: k_pairs_law's 32-bit counters cannot overflow */
#define PAIRS_STORE_BYTES (sizeof(int4) + sizeof(int2) + 1)

/* the passes ig_debug_pairs_time reports, in this order: the lift, the seven of a pixel build (LIFT_P_*), the law */
#define PAIRS_P_LIFT 0
#define PAIRS_P_BUILD 1
#define PAIRS_P_LAW (PAIRS_P_BUILD + LIFT_PASSES)
#define PAIRS_PASSES (PAIRS_P_LAW + 1)

static void pairs_free_staging(PairsBuf& p)
{
    for (int k = 0; k < 4; k++) hipFree(p.in[k]), p.in[k] = nullptr;
    for (int k = 0; k < 6; k++) hipFree(p.out_i[k]), p.out_i[k] = nullptr;
    for (int k = 0; k < 3; k++) hipFree(p.out_b[k]), p.out_b[k] = nullptr;
    hipFree(p.in_strands);
    p.in_strands = nullptr;
    p.piece_cap = 0;
}

static void free_pairs_buffers(ig_ctx* c)
{
    PairsBuf& p = c->pairs;
    hipFree(p.rowptr);
    hipFree(p.start);
    hipFree(p.iv);
    hipFree(p.bin_unit);
    hipFree(p.ends);
    hipFree(p.unit);
    hipFree(p.flag);
    hipFree(p.sc);
    hipFree(p.edges);
    hipFree(p.counts);
    pairs_free_staging(p);
    p = PairsBuf{};
}

/* FNV-1a over the 17 N words of the state: what a session is begun under and every later call of it finds again */
static int pairs_stamp(ig_ctx* c, unsigned long long* stamp)
{
    HIPCK(hipStreamSynchronize(c->stream));
    std::vector<int> host(17 * (size_t)c->N);
    HIPCK(hipMemcpy(host.data(), c->st_block, host.size() * sizeof(int), hipMemcpyDeviceToHost));
    unsigned long long h = 1469598103934665603ull;
    for (const int v : host) h = (h ^ (unsigned long long)(unsigned)v) * 1099511628211ull;
    *stamp = h;
    return 0;
}

/* what every call of a session but ig_pairs_end asks first */
static int pairs_usable(ig_ctx* c, const char* who)
{
    if (!c->pairs.live) return fail("%s: no session (ig_pairs_begin first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    if (!c->have_state) return fail("%s: upload a state first", who);
    unsigned long long now = 0;
    if (pairs_stamp(c, &now)) return -1;
    if (now != c->pairs.stamp) return fail("%s: the genome changed since ig_pairs_begin: the session's table is of another genome (ig_pairs_end, then begin again)", who);
    return 0;
}

/* room for `need` pairs in all: the three arrays made anew, the stored pairs copied over; a refusal leaves the store as it was */
static int pairs_grow_store(ig_ctx* c, const char* who, long long need)
{
    PairsBuf& p = c->pairs;
    if (need <= p.cap) return 0;
    if (need > PAIRS_MAX_STORE) return fail("%s: %lld pairs are more than a session stores (2^31 - 1)", who, need);
    const long long cap = std::min<long long>(std::max(need, p.cap + p.cap / 2), PAIRS_MAX_STORE);
    const unsigned long long bytes = (unsigned long long)cap * PAIRS_STORE_BYTES + (1ull << 20);
    size_t free_b = ~(size_t)0, total_b = 0;
    if (&hipMemGetInfo != nullptr) HIPCK(hipMemGetInfo(&free_b, &total_b));
    if (bytes > (unsigned long long)free_b) return fail("%s: a store of %lld pairs needs %llu bytes of device memory, %zu are free", who, cap, bytes, free_b);
    int4* ends = nullptr;
    int2* unit = nullptr;
    unsigned char* flag = nullptr;
    const int rc = [&]() -> int {
        DALLOC(ends, (size_t)cap);
        DALLOC(unit, (size_t)cap);
        DALLOC(flag, (size_t)cap);
        if (p.size > 0) {
            HIPCK(hipMemcpyAsync(ends, p.ends, (size_t)p.size * sizeof(int4), hipMemcpyDeviceToDevice, c->stream));
            HIPCK(hipMemcpyAsync(unit, p.unit, (size_t)p.size * sizeof(int2), hipMemcpyDeviceToDevice, c->stream));
            HIPCK(hipMemcpyAsync(flag, p.flag, (size_t)p.size, hipMemcpyDeviceToDevice, c->stream));
        }
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        hipFree(ends);
        hipFree(unit);
        hipFree(flag);
        return rc;
    }
    hipFree(p.ends);
    hipFree(p.unit);
    hipFree(p.flag);
    p.ends = ends, p.unit = unit, p.flag = flag, p.cap = cap;
    return 0;
}

static int pairs_reserve_piece(PairsBuf& p, long long n)
{
    if (n <= p.piece_cap) return 0;
    pairs_free_staging(p);
    for (int k = 0; k < 4; k++) DALLOC(p.in[k], (size_t)n);
    DALLOC(p.in_strands, (size_t)n);
    for (int k = 0; k < 6; k++) DALLOC(p.out_i[k], (size_t)n);
    for (int k = 0; k < 3; k++) DALLOC(p.out_b[k], (size_t)n);
    p.piece_cap = n;
    return 0;
}

extern "C" int ig_pairs_begin(ig_ctx* c, const int32_t* src_rowptr, int32_t n_contigs, const int32_t* src_start, const int32_t* src_end, const int32_t* new_start,
                              const int32_t* scaffold, const uint8_t* reversed, const int32_t* position, int64_t n_intervals, const int64_t* scaffold_len,
                              int32_t n_scaffolds, const int32_t* bin_unit, int64_t n_positions, int64_t n_bin_units, int64_t reserve_pairs)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pairs_begin";
    PairsBuf& p = c->pairs;
    if (p.live) return fail("%s: a session is open (ig_pairs_end first)", who);
    if (!c->have_state) return fail("%s: upload a state first", who);
    if (c->world != 1) return fail("%s: a pairs session needs the whole genome on one handle (this one holds shard %d of %d)", who, c->rank, c->world);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    const long long n = n_intervals, K = n_scaffolds, T = n_positions;
    if (n_contigs < 0 || n < 0 || n > 0x7fffffffll || K < 0 || T < 0 || T > 0x7fffffffll || n_bin_units < 0 || n_bin_units > T || reserve_pairs < 0)
        return fail("%s: bad sizes (%d contigs, %lld intervals, %lld scaffolds, %lld positions, %lld bins, reserve %lld)", who, n_contigs, n, K, T,
                    (long long)n_bin_units, (long long)reserve_pairs);
    if (K > (1ll << 30)) return fail("%s: %lld scaffolds are more than 2^30 (a record holds scaffold << 1 | reversed in 32 signed bits)", who, K);
    if (!src_rowptr || (n > 0 && (!src_start || !src_end || !new_start || !scaffold || !reversed || !position)) || (K > 0 && !scaffold_len) || (T > 0 && !bin_unit))
        return fail("%s: NULL argument", who);
    if (src_rowptr[0] != 0 || src_rowptr[n_contigs] != n) return fail("%s: src_rowptr runs from 0 to the number of intervals", who);
    for (int q = 0; q < n_contigs; q++)
        if (src_rowptr[q + 1] < src_rowptr[q]) return fail("%s: src_rowptr decreases behind contig %d", who, q);
    for (long long k = 0; k < K; k++)
        if (scaffold_len[k] < 0 || scaffold_len[k] > 0x7fffffffll) return fail("%s: scaffold %lld is %lld bp long: 0 .. 2^31 - 1", who, k, (long long)scaffold_len[k]);
    for (int q = 0; q < n_contigs; q++)
        for (long long i = src_rowptr[q]; i < src_rowptr[q + 1]; i++) {
            if (src_start[i] < 0 || src_end[i] < src_start[i]) return fail("%s: interval %lld is [%d, %d)", who, i, src_start[i], src_end[i]);
            if (i > src_rowptr[q] && src_start[i] < src_end[i - 1]) return fail("%s: intervals %lld and %lld of contig %d overlap or are not sorted", who, i - 1, i, q);
            if (scaffold[i] < -1 || scaffold[i] >= K) return fail("%s: interval %lld lies on scaffold %d of %lld", who, i, scaffold[i], K);
            if (scaffold[i] < 0) continue;
            if (position[i] < 0 || position[i] >= T) return fail("%s: interval %lld has position %d of %lld", who, i, position[i], T);
            if (new_start[i] < 0 || (long long)new_start[i] + (src_end[i] - src_start[i]) > scaffold_len[scaffold[i]])
                return fail("%s: interval %lld reaches beyond its scaffold (%d + %d of %lld bp)", who, i, new_start[i], src_end[i] - src_start[i], (long long)scaffold_len[scaffold[i]]);
        }
    for (long long r = 0; r < T; r++)
        if (bin_unit[r] < 0 || bin_unit[r] >= n_bin_units) return fail("%s: position %lld has bin unit %d of %lld", who, r, bin_unit[r], (long long)n_bin_units);
    unsigned long long stamp = 0;
    if (pairs_stamp(c, &stamp)) return -1;
    std::vector<PairsIv> iv((size_t)n);
    for (long long i = 0; i < n; i++)
        iv[(size_t)i] = PairsIv{src_end[i], new_start[i], scaffold[i] < 0 ? -1 : (int)(((unsigned)scaffold[i] << 1) | (reversed[i] ? 1u : 0u)), scaffold[i] < 0 ? -1 : position[i]};
    const int rc = [&]() -> int {
        DALLOC(p.rowptr, (size_t)n_contigs + 1);
        DALLOC(p.start, (size_t)n);
        DALLOC(p.iv, (size_t)n);
        DALLOC(p.bin_unit, (size_t)T);
        DALLOC(p.sc, (size_t)PAIRS_SC_WORDS);
        DALLOC(p.edges, (size_t)PAIRS_MAX_EDGES);
        DALLOC(p.counts, (size_t)4 * (PAIRS_MAX_EDGES - 1));
        HIPCK(hipMemcpyAsync(p.rowptr, src_rowptr, ((size_t)n_contigs + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (n > 0) {
            HIPCK(hipMemcpyAsync(p.start, src_start, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCK(hipMemcpyAsync(p.iv, iv.data(), (size_t)n * sizeof(PairsIv), hipMemcpyHostToDevice, c->stream));
        }
        if (T > 0) HIPCK(hipMemcpyAsync(p.bin_unit, bin_unit, (size_t)T * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        p.live = true; /* (pairs_grow_store fills a live session's store) */
        return pairs_grow_store(c, who, std::max<long long>(reserve_pairs, 1));
    }();
    if (rc) {
        free_pairs_buffers(c);
        return rc;
    }
    p.n_contigs = n_contigs, p.n_iv = n, p.K = (int)K, p.T = T, p.n_bin_units = n_bin_units;
    p.scaffold_len.assign(scaffold_len, scaffold_len + K);
    p.stamp = stamp;
    return 0;
}

/* One chunk: piece by piece through the staging arrays.  ms (may be null): the kernel's time, summed over the pieces, goes to
 * ms[PAIRS_P_LIFT].  On an error behind the first launch the store is what it was before the call. */
template <class Stage>
static int pairs_lift_staged(ig_ctx* c, const char* who, bool strands, long long n, Stage stage, int32_t* const out_i[6], uint8_t* const out_b[3], long long scalars[8],
                             LiftTimer& timer)
{
    PairsBuf& p = c->pairs;
    const bool want_out = out_b[2] != nullptr;
    if (pairs_grow_store(c, who, p.size + n)) return -1;
    if (pairs_reserve_piece(p, std::min<long long>(std::max<long long>(n, 1), PAIRS_PIECE))) return -1;
    const long long before = p.size;
    unsigned long long h_sc[PAIRS_SC_WORDS] = {0};
    h_sc[PAIRS_SC_CURSOR] = (unsigned long long)before;
    HIPCK(hipMemcpyAsync(p.sc, h_sc, sizeof(h_sc), hipMemcpyHostToDevice, c->stream));
    for (long long o = 0; o < n; o += PAIRS_PIECE) {
        const long long m = std::min<long long>(PAIRS_PIECE, n - o);
        if (stage(o, m)) return -1; /* the pairs o .. o + m - 1 into the staging arrays: a copy from the host, or ig_text_feed_pairs' conversion on the device */
        PairsOut out = {p.out_i[0], p.out_i[1], p.out_i[2], p.out_i[3], p.out_i[4], p.out_i[5], p.out_b[0], p.out_b[1], want_out ? p.out_b[2] : nullptr};
        const PairsStore store = {p.ends, p.unit, p.flag};
        timer.begin();
        hipLaunchKernelGGL(k_pairs_lift, dim3(lift_blocks(m)), dim3(PAIRS_THREADS), 0, c->stream, (const int*)p.in[0], (const int*)p.in[1], (const int*)p.in[2],
                           (const int*)p.in[3], strands ? (const unsigned char*)p.in_strands : (const unsigned char*)nullptr, m, (const int*)p.rowptr, p.n_contigs,
                           (const int*)p.start, (const PairsIv*)p.iv, out, store, p.sc + PAIRS_SC_CURSOR, (unsigned long long)p.cap, p.sc + PAIRS_SC_LIFT);
        timer.end(PAIRS_P_LIFT);
        if (want_out) {
            for (int k = 0; k < 6; k++) HIPCK(hipMemcpyAsync(out_i[k] + o, p.out_i[k], (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            for (int k = 0; k < 3; k++) HIPCK(hipMemcpyAsync(out_b[k] + o, p.out_b[k], (size_t)m, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCK(hipStreamSynchronize(c->stream)); /* (the staging arrays are the next piece's) */
    }
    HIPCK(hipMemcpy(h_sc, p.sc, sizeof(h_sc), hipMemcpyDeviceToHost));
    const unsigned long long* s = h_sc + PAIRS_SC_LIFT;
    if (s[PAIRS_IN] != (unsigned long long)n || s[PAIRS_KEPT] + s[PAIRS_MISS1] + s[PAIRS_MISS2] + s[PAIRS_UNPLACED] != (unsigned long long)n ||
        h_sc[PAIRS_SC_CURSOR] != (unsigned long long)before + s[PAIRS_KEPT] || h_sc[PAIRS_SC_CURSOR] > (unsigned long long)p.cap)
        return fail("%s: %llu pairs counted of %lld, %llu kept, the store's cursor at %llu of %lld (device error)", who, s[PAIRS_IN], n, s[PAIRS_KEPT],
                    h_sc[PAIRS_SC_CURSOR], p.cap);
    p.size = (long long)h_sc[PAIRS_SC_CURSOR];
    for (int k = 0; k < PAIRS_NS; k++) scalars[k] = (long long)s[k];
    scalars[5] = p.size;
    scalars[6] = scalars[7] = 0;
    return 0;
}

static int pairs_lift_impl(ig_ctx* c, const char* who, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, const uint8_t* strands, long long n,
                           int32_t* const out_i[6], uint8_t* const out_b[3], long long scalars[8], LiftTimer& timer)
{
    PairsBuf& p = c->pairs;
    const int32_t* in[4] = {c1, p1, c2, p2};
    return pairs_lift_staged(c, who, strands != nullptr, n, [&](long long o, long long m) -> int {
        for (int k = 0; k < 4; k++) HIPCK(hipMemcpyAsync(p.in[k], in[k] + o, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (strands) HIPCK(hipMemcpyAsync(p.in_strands, strands + o, (size_t)m, hipMemcpyHostToDevice, c->stream));
        return 0;
    }, out_i, out_b, scalars, timer);
}

extern "C" int ig_pairs_lift(ig_ctx* c, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, const uint8_t* strands, int64_t n,
                             int32_t* scaffold1, int32_t* pos1, int32_t* unit1, uint8_t* rev1, int32_t* scaffold2, int32_t* pos2, int32_t* unit2, uint8_t* rev2,
                             uint8_t* status, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pairs_lift";
    if (!scalars) return fail("%s: NULL output", who);
    if (n < 0 || (n > 0 && (!c1 || !p1 || !c2 || !p2))) return fail("%s: bad arguments (%lld pairs)", who, (long long)n);
    const int n_out = !!scaffold1 + !!pos1 + !!unit1 + !!rev1 + !!scaffold2 + !!pos2 + !!unit2 + !!rev2 + !!status;
    if (n_out != 0 && n_out != 9) return fail("%s: the nine per-pair outputs are given together or not at all", who);
    if (pairs_usable(c, who)) return -1;
    int32_t* const out_i[6] = {scaffold1, pos1, unit1, scaffold2, pos2, unit2};
    uint8_t* const out_b[3] = {rev1, rev2, status};
    long long sc[8];
    LiftTimer timer(c, nullptr, PAIRS_PASSES);
    if (pairs_lift_impl(c, who, c1, p1, c2, p2, strands, n, out_i, out_b, sc, timer)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    return 0;
}

/* The pixels of the store into the assembly-contacts snapshot; ms (may be null): LIFT_PASSES words.  scalars: the eight words of
 * assembly_contacts.SCALARS (entries: the stored pairs; nothing is unplaced in the store). */
static int pairs_pixels_impl(ig_ctx* c, const char* who, int kind, long long binsize, float* ms, long long* n_units, long long scalars[8])
{
    PairsBuf& p = c->pairs;
    LiftBuf& l = c->lift;
    long long U = 0;
    std::vector<int> first;
    if (kind == PAIRS_KIND_SUB) U = p.T;
    else if (kind == PAIRS_KIND_BIN) U = p.n_bin_units;
    else if (kind == PAIRS_KIND_SCAFFOLD) U = p.K;
    else if (kind == PAIRS_KIND_BINSIZE) {
        if (binsize < 1 || binsize > 0x7fffffffll) return fail("%s: a bin size is 1 .. 2^31 - 1 bp (got %lld)", who, binsize);
        first.resize((size_t)p.K);
        for (int k = 0; k < p.K; k++) { /* zoom_levels.bins_per_scaffold */
            first[(size_t)k] = (int)U;
            U += std::max<long long>(1, (p.scaffold_len[(size_t)k] + binsize - 1) / binsize);
            if (U > 0x7fffffffll) return fail("%s: bins of %lld bp are more than 2^31 - 1 units", who, binsize);
        }
    } else
        return fail("%s: kind is 0 (sub), 1 (bin), 2 (a bin size) or 3 (scaffold), got %d", who, kind);
    { /* the rows' counters, cursors and starts, before anything is allocated by their number */
        const unsigned long long need = (unsigned long long)(U + 2) * 32 + (1ull << 20);
        size_t free_b = ~(size_t)0, total_b = 0;
        if (&hipMemGetInfo != nullptr) HIPCK(hipMemGetInfo(&free_b, &total_b));
        if (need > (unsigned long long)free_b) return fail("%s: %lld units need %llu bytes of device memory, %zu are free (a larger bin size)", who, U, need, free_b);
    }
    int* d_first = nullptr;
    const int rc = [&]() -> int {
        const int* tab = p.bin_unit;
        if (kind == PAIRS_KIND_BINSIZE) {
            DALLOC(d_first, (size_t)p.K);
            if (p.K > 0) HIPCK(hipMemcpyAsync(d_first, first.data(), (size_t)p.K * sizeof(int), hipMemcpyHostToDevice, c->stream));
            tab = d_first;
        }
        const int Ui = (int)U;
        const long long S = p.size;
        unsigned long long* d_sc = p.sc + PAIRS_SC_EMIT;
        HIPCK(hipMemsetAsync(d_sc, 0, 2 * sizeof(unsigned long long), c->stream));
        const PairsStore store = {p.ends, p.unit, p.flag};
        auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
            if (S == 0) return; /* an empty store: nothing to launch, the rows stay empty */
            const dim3 grid(lift_blocks(S)), block(PAIRS_THREADS);
            if (!scatter) hipLaunchKernelGGL((k_pairs_emit<false>), grid, block, 0, c->stream, store, S, kind, (unsigned)binsize, tab, Ui, slots, ent, n_ent, d_sc);
            else hipLaunchKernelGGL((k_pairs_emit<true>), grid, block, 0, c->stream, store, S, kind, (unsigned)binsize, tab, Ui, slots, ent, n_ent, d_sc);
        };
        auto check = [&](long long E) { return E != S ? fail("%s: %lld entries of %lld stored pairs (a unit outside 0 .. %lld: inconsistent tables)", who, E, S, U - 1) : 0; };
        /* per entry: the word, the long rows' scratch and their runs' items (8 bytes each), a bit, a summed entry (12 bytes) */
        const RowsSpec spec = {d_sc, 2, 0, 37, " (the pixels' temporaries: a larger bin size makes fewer rows, not fewer entries)", true,
                               {LIFT_P_COUNT, LIFT_P_SCAN, LIFT_P_SCATTER, LIFT_P_SORT_SHORT, LIFT_P_REDUCE}};
        LiftTimer timer(c, ms, LIFT_PASSES);
        unsigned long long h_sc[2];
        long long E = 0, n_out = 0;
        if (rows_build(c, who, l.rows, Ui, spec, h_sc, check, emit, timer, l.forms, &E, &n_out)) return -1;
        HIPCK(hipStreamSynchronize(c->stream));
        l.level = 2;
        l.n_units = U;
        l.n_entries = n_out;
        l.n_placed = p.T;
        l.contacts_kept = S;
        l.unplaced[0] = l.unplaced[1] = 0;
        const long long sc[8] = {S, E, S, 0, 0, p.T, U, n_out};
        for (int k = 0; k < 8; k++) scalars[k] = sc[k];
        return 0;
    }();
    hipStreamSynchronize(c->stream);
    hipFree(d_first);
    rows_free_temp(l.rows);
    if (rc) {
        lift_release_snapshot(c);
        return rc;
    }
    l.valid = true;
    *n_units = U;
    return 0;
}

extern "C" int ig_pairs_pixels_build(ig_ctx* c, int32_t kind, int64_t binsize, int64_t* n_units, int64_t* n_entries, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pairs_pixels_build";
    lift_release_snapshot(c); /* whatever happens, the result of an earlier build is gone */
    if (!n_units || !n_entries || !scalars) return fail("%s: NULL output", who);
    if (pairs_usable(c, who)) return -1;
    long long U = 0, sc[8];
    if (pairs_pixels_impl(c, who, kind, binsize, nullptr, &U, sc)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_units = U;
    *n_entries = c->lift.n_entries;
    return 0;
}

/* counts: [4][n_edges - 1] on the host.  scalars: the stored pairs, those counted (both ends on one scaffold), the others */
static int pairs_law_impl(ig_ctx* c, const char* who, const int64_t* edges_bp, int n_edges, int flip, int64_t* counts, long long scalars[8], LiftTimer& timer)
{
    PairsBuf& p = c->pairs;
    if (n_edges < 2 || n_edges > PAIRS_MAX_EDGES) return fail("%s: 2 <= n_edges <= %d (got %d)", who, PAIRS_MAX_EDGES, n_edges);
    if (!edges_bp || !counts) return fail("%s: NULL argument", who);
    for (int k = 0; k < n_edges; k++)
        if (edges_bp[k] < 0 || (k > 0 && edges_bp[k] < edges_bp[k - 1])) return fail("%s: the edges are >= 0 and ascending (edge %d is %lld)", who, k, (long long)edges_bp[k]);
    const size_t words = (size_t)4 * (size_t)(n_edges - 1);
    HIPCK(hipMemcpyAsync(p.edges, edges_bp, (size_t)n_edges * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemsetAsync(p.counts, 0, words * sizeof(unsigned long long), c->stream));
    const PairsStore store = {p.ends, p.unit, p.flag};
    timer.begin();
    if (p.size > 0)
        hipLaunchKernelGGL(k_pairs_law, dim3(lift_blocks(p.size)), dim3(PAIRS_THREADS), 0, c->stream, store, p.size, (const long long*)p.edges, n_edges, flip ? 1 : 0, p.counts);
    timer.end(PAIRS_P_LAW);
    HIPCK(hipMemcpyAsync(counts, p.counts, words * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    long long cis = 0;
    for (size_t k = 0; k < words; k++) cis += counts[k];
    if (cis < 0 || cis > p.size) return fail("%s: %lld pairs counted of %lld stored (device error)", who, cis, p.size);
    const long long sc[8] = {p.size, cis, p.size - cis, 0, 0, 0, 0, 0};
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    return 0;
}

extern "C" int ig_pairs_law(ig_ctx* c, const int64_t* edges_bp, int32_t n_edges, int32_t flip_strands, int64_t* counts, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pairs_law";
    if (!scalars) return fail("%s: NULL output", who);
    if (pairs_usable(c, who)) return -1;
    long long sc[8];
    LiftTimer timer(c, nullptr, PAIRS_PASSES);
    if (pairs_law_impl(c, who, edges_bp, n_edges, flip_strands, counts, sc, timer)) return -1;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    return 0;
}

/* empties the store: the table and the buffers stay */
extern "C" int ig_pairs_clear(ig_ctx* c)
{
    IG_JOIN(c);
    if (!c->pairs.live) return fail("ig_pairs_clear: no session (ig_pairs_begin first)");
    c->pairs.size = 0;
    return 0;
}

extern "C" int ig_pairs_end(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->pairs.live) return fail("ig_pairs_end: no session (ig_pairs_begin first)");
    HIPCK(hipStreamSynchronize(c->stream));
    free_pairs_buffers(c);
    return 0;
}

/* The three passes n times, hipEvents around each: every repeat empties the store, lifts the chunk (no per-pair outputs), builds the
 * pixels and counts the law; ms_n[n][PAIRS_PASSES] = {lift, count, scan, scatter, sort_short, sort_lds, sort_long, reduce, law}.  Behind
 * it the store holds the chunk once and the snapshot its pixels.  *checksum (may be NULL): the scalars and the histogram of the last
 * repeat, each word weighted by its place. */
extern "C" int ig_debug_pairs_time(ig_ctx* c, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, const uint8_t* strands, int64_t n_pairs,
                                   int32_t kind, int64_t binsize, const int64_t* edges_bp, int32_t n_edges, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_pairs_time";
    lift_release_snapshot(c);
    if (n < 1 || !ms_n || n_pairs < 0 || (n_pairs > 0 && (!c1 || !p1 || !c2 || !p2))) return fail("%s: bad arguments", who);
    if (n_edges < 2 || n_edges > PAIRS_MAX_EDGES || !edges_bp) return fail("%s: 2 <= n_edges <= %d", who, PAIRS_MAX_EDGES);
    if (pairs_usable(c, who)) return -1;
    int32_t* const no_i[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint8_t* const no_b[3] = {nullptr, nullptr, nullptr};
    std::vector<int64_t> counts((size_t)4 * (size_t)(n_edges - 1));
    long long sc[3][8], U = 0;
    for (int r = 0; r < n; r++) {
        float* ms = ms_n + (size_t)r * PAIRS_PASSES;
        c->pairs.size = 0;
        LiftTimer timer(c, ms, PAIRS_PASSES);
        if (pairs_lift_impl(c, who, c1, p1, c2, p2, strands, n_pairs, no_i, no_b, sc[0], timer)) return -1;
        if (pairs_law_impl(c, who, edges_bp, n_edges, 1, counts.data(), sc[2], timer)) return -1;
        float build[LIFT_PASSES];
        lift_release_snapshot(c);
        if (pairs_pixels_impl(c, who, kind, binsize, build, &U, sc[1])) return -1;
        for (int k = 0; k < LIFT_PASSES; k++) ms[PAIRS_P_BUILD + k] = build[k];
    }
    if (checksum) {
        std::vector<long long> h;
        for (int q = 0; q < 3; q++) h.insert(h.end(), sc[q], sc[q] + 8);
        h.insert(h.end(), counts.begin(), counts.end());
        *checksum = (long long)weighted_checksum(h.data(), h.size());
    }
    return 0;
}
