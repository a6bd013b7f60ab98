/* ig_host_emap.inc -- part of ig_hip.hip (one translation unit; included there in order): the expected contact map of the current
 * genome (ig_kernels_emap.cuh; the rule: instagraal_amd/expected_map.py). */

/* the forms of ig_debug_expected_map_form */
#define EMAP_FORM_DEFAULT 0
#define EMAP_FORM_ROWS 1
#define EMAP_FORM_TILES 2
#define EMAP_FORM_TILES_PLAIN 3 /* the tiles without the constant shortcut */

/* The form ig_expected_map runs unless ig_debug_expected_map_form says otherwise: the tile form from this many positions per pixel
 * on (0: never), the row form (the yardstick) below; at bin == 1 a tile holds one pair and the row form runs whatever this says.
 * The figures behind the value: tools/expected_map_bench.py -> profiles/r12_expected_map.json, DESIGN.md 4.15. */
#define EMAP_TILE_MIN_BIN 0

static void free_emap_buffers(ig_ctx* c)
{
    EmapBuf& e = c->emap;
    hipFree(e.img);
    hipFree(e.sc);
    hipFree(e.cnt);
    hipFree(e.off);
    hipFree(e.tot);
    hipFree(e.list);
    const int form = e.form;
    e = EmapBuf{};
    e.form = form; /* (the setting of ig_debug_expected_map_form belongs to the handle and stays) */
}

/* the genome view under this entry point's name: the pixels under max_side, ds and meta by position (no contact is read, so no
 * record is asked for) */
static int emap_view(ig_ctx* c, const char* who, int max_side, int* T, int* bin, int* side)
{
    if (max_side < 1) return fail("%s: max_side must be >= 1 (got %d)", who, max_side);
    GenomeDims d;
    if (genome_view(c, who, max_side, GENOME_SORTED, &d)) return -1;
    if (!c->have_params) return fail("%s: set parameters first", who);
    *T = d.T;
    *bin = d.bin;
    *side = d.side;
    return 0;
}

static inline bool emap_tiles(int form, int bin)
{
    if (bin <= 1) return false;
    if (form == EMAP_FORM_DEFAULT) return EMAP_TILE_MIN_BIN > 0 && bin >= EMAP_TILE_MIN_BIN;
    return form != EMAP_FORM_ROWS;
}

/* the images and the scalars of one call (side > 0) */
static int emap_alloc(ig_ctx* c, int side, bool tiles)
{
    EmapBuf& e = c->emap;
    free_emap_buffers(c);
    DALLOC(e.sc, (size_t)EMAP_NS);
    DALLOC(e.img, 3 * (size_t)side * (size_t)side);
    if (tiles) {
        DALLOC(e.cnt, (size_t)side);
        DALLOC(e.off, (size_t)side + 1);
        DALLOC(e.tot, (size_t)scan_chunks(side));
    }
    return 0;
}

/* One build on the library's stream: zero, the scalars (and the tile counts), the row form or the work list and the tile form, the
 * mirror of every image.  The tile form waits once, for the size of its list. */
static int emap_enqueue(ig_ctx* c, const char* who, int T, int bin, int side, int form)
{
    EmapBuf& e = c->emap;
    const size_t px = (size_t)side * (size_t)side;
    const bool tiles = emap_tiles(form, bin);
    unsigned long long *cis_q = e.img, *cis_pairs = e.img + px, *ring_pairs = e.img + 2 * px;
    HIPCK(hipMemsetAsync(e.img, 0, 3 * px * sizeof(unsigned long long), c->stream));
    HIPCK(hipMemsetAsync(e.sc, 0, EMAP_NS * sizeof(unsigned long long), c->stream));
    const int blocks = (T + EMAP_THREADS - 1) / EMAP_THREADS;
    hipLaunchKernelGGL(k_emap_count, dim3(blocks), dim3(EMAP_THREADS), 0, c->stream, c->genome.ds, c->genome.meta, T, bin, tiles ? e.cnt : nullptr, e.sc);
    if (!tiles) {
        hipLaunchKernelGGL(k_emap_rows, dim3(blocks), dim3(EMAP_THREADS), 0, c->stream, c->genome.ds, c->genome.meta, T, bin, side, c->glob, cis_q, cis_pairs, ring_pairs, e.sc);
    } else {
        HIPCK(hipMemsetAsync(e.off, 0, sizeof(unsigned long long), c->stream));
        scan64_enqueue(c, e.cnt, e.off + 1, 0, side, 1, e.tot);
        unsigned long long n_tiles = 0, nonmono = 0;
        HIPCK(hipMemcpyAsync(&n_tiles, e.off + side, sizeof(n_tiles), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(&nonmono, e.sc + EMAP_SC_NONMONO, sizeof(nonmono), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        /* every pixel lists itself at least, nobody more than the pixels from itself on: checked before anything is sized by it */
        const unsigned long long most = (unsigned long long)side * ((unsigned long long)side + 1) / 2;
        if (n_tiles < (unsigned long long)side || n_tiles > most)
            return fail("%s: a work list of %llu tiles for an image of %d pixels a side (inconsistent tables)", who, n_tiles, side);
        if (n_tiles > e.list_cap) {
            hipFree(e.list);
            e.list = nullptr;
            e.list_cap = 0;
            DALLOC(e.list, (size_t)n_tiles);
            e.list_cap = n_tiles;
        }
        hipLaunchKernelGGL(k_emap_list, dim3((unsigned)((n_tiles + EMAP_THREADS - 1) / EMAP_THREADS)), dim3(EMAP_THREADS), 0, c->stream, e.off, side, (long long)n_tiles, e.list);
        /* the shortcut leans on ds not decreasing inside a contig: where k_emap_count saw it decrease every tile is walked */
        if (form != EMAP_FORM_TILES_PLAIN && !nonmono)
            hipLaunchKernelGGL((k_emap_tiles<true>), dim3((unsigned)n_tiles), dim3(EMAP_THREADS), 0, c->stream, e.list, c->genome.ds, c->genome.meta, T, bin, side, c->glob, cis_q, cis_pairs,
                               ring_pairs, e.sc);
        else
            hipLaunchKernelGGL((k_emap_tiles<false>), dim3((unsigned)n_tiles), dim3(EMAP_THREADS), 0, c->stream, e.list, c->genome.ds, c->genome.meta, T, bin, side, c->glob, cis_q, cis_pairs,
                               ring_pairs, e.sc);
    }
    const int nt = (side + MAP_TILE - 1) / MAP_TILE; /* (the contact map's mirror, ig_kernels_map.cuh) */
    for (int k = 0; k < 3; k++) hipLaunchKernelGGL(k_map_mirror, dim3(nt, nt), dim3(MAP_TILE, 8), 0, c->stream, e.img + (size_t)k * px, side);
    return 0;
}

/* the scalars behind a build, and the overflow guard: a pixel holds at most bin^2 pairs, twice on the diagonal, each of at most
 * max(max_q, q_trans) -- what expected_map.compose adds per pair */
static int emap_finish(ig_ctx* c, const char* who, int T, int bin, long long scalars[8])
{
    unsigned long long sc[EMAP_NS];
    HIPCK(hipMemcpyAsync(sc, c->emap.sc, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    const long long qt = ig_quantize((double)c->par_model.v_inter);
    const unsigned long long big = std::max(sc[EMAP_SC_MAXQ], (unsigned long long)(qt < 0 ? -qt : qt));
    const unsigned long long n = 2ull * (unsigned long long)bin * (unsigned long long)bin; /* bin <= T < 2^31 */
    if (big > ((1ull << 62) - 1) / n) /* big * n >= 2^62 */
        return fail("%s: model value too large for this pixel size (the largest value, %.6g, times %llu pairs does not fit the 64-bit sum)", who, (double)big / IG_QSCALE, n);
    for (int k = 0; k < 8; k++) scalars[k] = 0;
    scalars[0] = T;
    scalars[1] = (long long)sc[EMAP_SC_LINEAR];
    scalars[2] = (long long)sc[EMAP_SC_RING];
    scalars[3] = (long long)sc[EMAP_SC_MAXQ];
    scalars[4] = (long long)sc[EMAP_SC_TILES_EVAL];
    scalars[5] = (long long)sc[EMAP_SC_TILES_CONST];
    return 0;
}

static int emap_run(ig_ctx* c, int32_t max_side, int64_t* cis_q, int64_t* cis_pairs, int64_t* ring_pairs, int64_t image_capacity, int32_t* side_out, int32_t* bin_out,
                    int64_t scalars[8])
{
    const char* who = "ig_expected_map";
    int T = 0, bin = 1, side = 0;
    if (emap_view(c, who, max_side, &T, &bin, &side)) return -1;
    *side_out = side;
    *bin_out = bin;
    const long long px = (long long)side * (long long)side;
    if (image_capacity < px) return fail("%s: an image needs %d x %d = %lld entries, the caller's buffers hold %lld", who, side, side, px, (long long)image_capacity);
    for (int k = 0; k < 8; k++) scalars[k] = 0;
    if (px == 0) return 0;
    if (!cis_q || !cis_pairs || !ring_pairs) return fail("%s: an image is NULL", who);
    if (emap_alloc(c, side, emap_tiles(c->emap.form, bin))) return -1;
    if (emap_enqueue(c, who, T, bin, side, c->emap.form)) return -1;
    long long sc[8];
    if (emap_finish(c, who, T, bin, sc)) return -1;
    const EmapBuf& e = c->emap;
    HIPCK(hipMemcpyAsync(cis_q, e.img, (size_t)px * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(cis_pairs, e.img + px, (size_t)px * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(ring_pairs, e.img + 2 * px, (size_t)px * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    return 0;
}

extern "C" int ig_expected_map(ig_ctx* c, int32_t max_side, int64_t* cis_q, int64_t* cis_pairs, int64_t* ring_pairs, int64_t image_capacity, int32_t* side,
                               int32_t* bin, int64_t scalars[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!side || !bin || !scalars) return fail("ig_expected_map: NULL output");
    const int rc = emap_run(c, max_side, cis_q, cis_pairs, ring_pairs, image_capacity, side, bin, scalars);
    free_emap_buffers(c); /* whatever happened: nothing of the feature outlives the call */
    return rc;
}

extern "C" int ig_debug_expected_map_form(ig_ctx* c, int32_t form)
{
    IG_JOIN(c);
    if (form < EMAP_FORM_DEFAULT || form > EMAP_FORM_TILES_PLAIN) return fail("ig_debug_expected_map_form: 0 default, 1 rows, 2 tiles, 3 tiles without the constant shortcut (got %d)", form);
    c->emap.form = form;
    return 0;
}

static int emap_time(ig_ctx* c, int32_t max_side, int32_t form, int32_t n, float* ms_n, int64_t* checksum)
{
    const char* who = "ig_debug_expected_map_time";
    int T = 0, bin = 1, side = 0;
    if (emap_view(c, who, max_side, &T, &bin, &side)) return -1;
    if (side == 0) return fail("%s: no sub-fragment is placed", who);
    if (emap_alloc(c, side, emap_tiles(form, bin))) return -1;
    if (time_repeats(c, who, n, ms_n, [&] { return emap_enqueue(c, who, T, bin, side, form); })) return -1;
    long long sc[8];
    if (emap_finish(c, who, T, bin, sc)) return -1;
    if (checksum) { /* of the last build: the three images word by word, then the pair counts and the largest value: every form must agree on it */
        EmapBuf& e = c->emap;
        const long long words = 3 * (long long)side * (long long)side;
        HIPCK(hipMemsetAsync(e.sc, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_emap_checksum, dim3((unsigned)std::min<long long>((words + EMAP_THREADS - 1) / EMAP_THREADS, 4096)), dim3(EMAP_THREADS), 0, c->stream, e.img, words, e.sc);
        unsigned long long s = 0;
        HIPCK(hipMemcpyAsync(&s, e.sc, sizeof(s), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        for (int k = 1; k <= 3; k++) s += (unsigned long long)sc[k] * (unsigned long long)(words + k);
        *checksum = (long long)s;
    }
    return 0;
}

extern "C" int ig_debug_expected_map_time(ig_ctx* c, int32_t max_side, int32_t form, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n < 1 || !ms_n) return fail("ig_debug_expected_map_time: bad arguments");
    if (form < EMAP_FORM_DEFAULT || form > EMAP_FORM_TILES_PLAIN) return fail("ig_debug_expected_map_time: 0 default, 1 rows, 2 tiles, 3 tiles without the constant shortcut (got %d)", form);
    const int rc = emap_time(c, max_side, form, n, ms_n, checksum);
    free_emap_buffers(c);
    return rc;
}
