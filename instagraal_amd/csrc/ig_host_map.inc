/* ig_host_map.inc -- part of ig_hip.hip (one translation unit; included there in order): the contact map of the current genome (display_current_matrix CL:2555-2605): the order of the placed sub-fragments, the binned image. */

static void free_map_buffers(ig_ctx* c)
{
    hipFree(c->map.base);
    hipFree(c->map.pix);
    hipFree(c->map.order);
    hipFree(c->map.err);
    hipFree(c->map.image);
    c->map = MapBuf{};
}

/* binning rule: bin = max(1, ceil(T / max_side)) positions per pixel, side = ceil(T / bin) pixels */
static void map_binning(long long T, long long max_side, int* bin, int* side)
{
    const long long b = std::max<long long>(1, (T + max_side - 1) / max_side);
    *bin = (int)b;
    *side = (int)((T + b - 1) / b);
}

/* The pixel table of the current genome (and, want_order, the order itself) on the device.
 * Contigs in ascending order of their canonical id (what ig_download_state returns, CL:2715-2881; the reference walks np.unique of
 * its contig ids, CL:2563-2567), a contig only if every one of its bins is active (CL:2571); inside a contig the rank of a
 * sub-fragment is Tables.cp[s].y.  The numbering of the contigs is the host's (canonical_ids: a stable sort of the contig heads by
 * length, as ig_download_state does it) on the N-length state; everything M-length happens in k_map_pixels on the live tables. */
static int map_prepare(ig_ctx* c, const char* who, long long max_side, bool want_order, int* T_out, int* bin_out, int* side_out)
{
    if (!c->have_state || !c->have_sub) return fail("%s: the sub-fragment table and a state are required", who);
    if (c->nuis_in_flight) return fail("%s: a nuisance step is in flight (ig_nuis_end first)", who);
    if (c->chain_busy) return fail("%s: a chain is in flight (ig_nuis_chain_end first)", who);
    const size_t n = (size_t)c->N;
    const int M = c->M;
    HIPCK(hipStreamSynchronize(c->stream));
    std::vector<int> host(17 * n);
    HIPCK(hipMemcpy(host.data(), c->st_block, 17 * n * sizeof(int), hipMemcpyDeviceToHost));
    const int *pos = &host[0], *cid = &host[2 * n], *L = &host[7 * n], *SL = &host[8 * n], *activ = &host[15 * n];
    std::vector<int> ids;
    int nc = 0;
    canonical_ids(pos, cid, L, n, ids, &nc);
    std::vector<long long> first((size_t)nc + 1, 0); /* sub-fragments of contig id, then its first position (-1: not placed) */
    std::vector<char> placed((size_t)nc, 1);
    for (size_t f = 0; f < n; f++) {
        if (ids[f] < 0 || ids[f] >= nc) return fail("%s: a bin belongs to no contig head (inconsistent state)", who);
        if (pos[f] == 0) first[(size_t)ids[f]] = SL[f];
        if (activ[f] != 1) placed[(size_t)ids[f]] = 0;
    }
    long long T = 0;
    for (int k = 0; k < nc; k++) {
        const long long len = first[(size_t)k];
        first[(size_t)k] = placed[(size_t)k] ? T : -1;
        if (placed[(size_t)k]) T += len;
    }
    if (T > M) return fail("%s: the placed contigs hold %lld sub-fragments, the table has %d (inconsistent state)", who, T, M);
    std::vector<int> base(n);
    for (size_t f = 0; f < n; f++) base[f] = (int)first[(size_t)ids[f]];
    MapBuf& m = c->map;
    if (m.N != c->N || m.M != M) {
        free_map_buffers(c);
        DALLOC(m.base, n);
        DALLOC(m.pix, (size_t)M);
        DALLOC(m.order, (size_t)M);
        DALLOC(m.err, 1);
        m.N = c->N;
        m.M = M;
    }
    int bin = 1, side = 0;
    map_binning(T, max_side, &bin, &side);
    *T_out = (int)T;
    *bin_out = bin;
    *side_out = side;
    HIPCK(hipMemcpyAsync(m.base, base.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemsetAsync(m.err, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_map_pixels, dim3((M + 255) / 256), dim3(256), 0, c->stream, c->sub_tab, c->tab, m.base, M, (int)T, bin, m.pix,
                       want_order ? m.order : nullptr, m.err);
    int err = 0;
    HIPCK(hipMemcpyAsync(&err, m.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream)); /* (`base` is pageable host memory of this frame) */
    if (err) return fail("%s: the coordinate tables and the state disagree (a rank beyond its contig)", who);
    return 0;
}

extern "C" int ig_contact_map_order(ig_ctx* c, int32_t* order_M, int32_t* n_placed)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!order_M || !n_placed) return fail("ig_contact_map_order: NULL output");
    int T = 0, bin = 1, side = 0;
    if (map_prepare(c, "ig_contact_map_order", 1, true, &T, &bin, &side)) return -1;
    if (T > 0) HIPCK(hipMemcpy(order_M, c->map.order, (size_t)T * sizeof(int), hipMemcpyDeviceToHost));
    *n_placed = T;
    return 0;
}

/* zero + accumulate (+ mirror) on the library's stream; the pixel table is in place */
static int map_enqueue_pass(ig_ctx* c, int side, bool combine)
{
    MapBuf& m = c->map;
    const size_t px = (size_t)side * (size_t)side;
    HIPCK(hipMemsetAsync(m.image, 0, px * sizeof(unsigned long long), c->stream));
    if (c->Z > 0) {
        const int blocks = (int)std::min<long long>((c->Z + MAP_THREADS - 1) / MAP_THREADS, 4096);
        const bool narrow = c->max_count < (1 << 25); /* 64 counts fit an int */
        if (combine && narrow)
            hipLaunchKernelGGL((k_contact_map<true, int>), dim3(blocks), dim3(MAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, m.pix, side, m.image, c->rank, c->world);
        else if (combine)
            hipLaunchKernelGGL((k_contact_map<true, long long>), dim3(blocks), dim3(MAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, m.pix, side, m.image, c->rank, c->world);
        else
            hipLaunchKernelGGL((k_contact_map<false, int>), dim3(blocks), dim3(MAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, m.pix, side, m.image, c->rank, c->world);
    }
    if (combine) {
        const int nt = (side + MAP_TILE - 1) / MAP_TILE;
        hipLaunchKernelGGL(k_map_mirror, dim3(nt, nt), dim3(MAP_TILE, 8), 0, c->stream, m.image, side);
    }
    return 0;
}

static int map_ensure_image(ig_ctx* c, int side)
{
    MapBuf& m = c->map;
    const size_t px = (size_t)side * (size_t)side;
    if (px > m.image_cap) {
        hipFree(m.image);
        m.image = nullptr;
        m.image_cap = 0;
        DALLOC(m.image, px);
        m.image_cap = px;
    }
    return 0;
}

extern "C" int ig_contact_map(ig_ctx* c, int32_t max_side, int64_t* image, int64_t image_capacity, int32_t* side_out, int32_t* bin_out)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (max_side < 1) return fail("ig_contact_map: max_side must be >= 1 (got %d)", max_side);
    if (!side_out || !bin_out) return fail("ig_contact_map: NULL output");
    if (!c->have_contacts) return fail("ig_contact_map: upload the contacts first");
    int T = 0, bin = 1, side = 0;
    if (map_prepare(c, "ig_contact_map", max_side, false, &T, &bin, &side)) return -1;
    *side_out = side;
    *bin_out = bin;
    const long long px = (long long)side * (long long)side;
    if (image_capacity < px) return fail("ig_contact_map: the image needs %d x %d = %lld entries, the caller's buffer holds %lld", side, side, px, (long long)image_capacity);
    if (px == 0) return 0;
    if (!image) return fail("ig_contact_map: image is NULL");
    if (map_ensure_image(c, side)) return -1;
    if (map_enqueue_pass(c, side, true)) return -1;
    HIPCK(hipMemcpyAsync(image, c->map.image, (size_t)px * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ig_debug_contact_map_time(ig_ctx* c, int32_t max_side, int32_t combine, int32_t n, float* ms_n, int64_t* image_sum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (max_side < 1 || n < 1 || !ms_n) return fail("ig_debug_contact_map_time: bad arguments");
    if (!c->have_contacts) return fail("ig_debug_contact_map_time: upload the contacts first");
    int T = 0, bin = 1, side = 0;
    if (map_prepare(c, "ig_debug_contact_map_time", max_side, false, &T, &bin, &side)) return -1;
    if (side == 0) return fail("ig_debug_contact_map_time: no sub-fragment is placed");
    if (map_ensure_image(c, side)) return -1;
    hipEvent_t a, b;
    HIPCK(hipEventCreate(&a));
    HIPCK(hipEventCreate(&b));
    int rc = 0;
    for (int r = 0; r < n && !rc; r++) {
        hipError_t e = hipEventRecord(a, c->stream);
        rc = map_enqueue_pass(c, side, combine != 0);
        if (e == hipSuccess) e = hipEventRecord(b, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_n[r], a, b);
        if (e != hipSuccess && !rc) rc = fail("ig_debug_contact_map_time: %s", hipGetErrorString(e));
    }
    hipEventDestroy(a);
    hipEventDestroy(b);
    if (rc) return rc;
    if (image_sum) { /* the sum of the last image: both forms of the kernel must agree on it */
        const size_t px = (size_t)side * (size_t)side;
        std::vector<long long> h(px);
        HIPCK(hipMemcpy(h.data(), c->map.image, px * sizeof(long long), hipMemcpyDeviceToHost));
        long long s = 0;
        for (long long v : h) s += v;
        *image_sum = s;
    }
    return 0;
}
