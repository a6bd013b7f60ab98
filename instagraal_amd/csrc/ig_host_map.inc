/* ig_host_map.inc -- part of ig_hip.hip (one translation unit; included there in order): the contact map of the current genome
 * (display_current_matrix CL:2555-2605): the order of the placed sub-fragments, the binned image over the pixel table of the genome
 * view (ig_host_genome.inc).  k_map_mirror and MAP_TILE serve the expected map too (ig_host_emap.inc). */

static void free_map_buffers(ig_ctx* c)
{
    hipFree(c->map.image);
    c->map = MapBuf{};
}

extern "C" int ig_contact_map_order(ig_ctx* c, int32_t* order_M, int32_t* n_placed)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!order_M || !n_placed) return fail("ig_contact_map_order: NULL output");
    GenomeDims d;
    if (genome_view(c, "ig_contact_map_order", 1, GENOME_ORDER, &d)) return -1;
    if (d.T > 0) HIPCK(hipMemcpy(order_M, c->genome.order, (size_t)d.T * sizeof(int), hipMemcpyDeviceToHost));
    *n_placed = d.T;
    return 0;
}

/* zero + accumulate (+ mirror) on the library's stream; the pixel table (genome.pix) is in place */
static int map_enqueue_pass(ig_ctx* c, int side, bool combine)
{
    MapBuf& m = c->map;
    const int* pix = c->genome.pix;
    const size_t px = (size_t)side * (size_t)side;
    HIPCK(hipMemsetAsync(m.image, 0, px * sizeof(unsigned long long), c->stream));
    if (c->Z > 0) {
        const int blocks = (int)std::min<long long>((c->Z + MAP_THREADS - 1) / MAP_THREADS, 4096);
        const bool narrow = c->max_count < (1 << 25); /* 64 counts fit an int */
        if (combine && narrow)
            hipLaunchKernelGGL((k_contact_map<true, int>), dim3(blocks), dim3(MAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, pix, side, m.image, c->rank, c->world);
        else if (combine)
            hipLaunchKernelGGL((k_contact_map<true, long long>), dim3(blocks), dim3(MAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, pix, side, m.image, c->rank, c->world);
        else
            hipLaunchKernelGGL((k_contact_map<false, int>), dim3(blocks), dim3(MAP_THREADS), 0, c->stream, c->crow, c->cc, c->Z, pix, side, m.image, c->rank, c->world);
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
    GenomeDims d;
    if (genome_view(c, "ig_contact_map", max_side, 0, &d)) return -1;
    const int side = d.side;
    *side_out = side;
    *bin_out = d.bin;
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
    GenomeDims d;
    if (genome_view(c, "ig_debug_contact_map_time", max_side, 0, &d)) return -1;
    const int side = d.side;
    if (side == 0) return fail("ig_debug_contact_map_time: no sub-fragment is placed");
    if (map_ensure_image(c, side)) return -1;
    if (time_repeats(c, "ig_debug_contact_map_time", n, ms_n, [&] { return map_enqueue_pass(c, side, combine != 0); })) return -1;
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
