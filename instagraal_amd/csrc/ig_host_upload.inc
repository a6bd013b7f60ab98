/* ig_host_upload.inc -- part of ig_hip.hip (one translation unit; included there in order): uploads (contacts -> CSR + packed + tiled copies, sub-fragment table, state, parameters, initial genome), downloads, contig bookkeeping, the full likelihood. */

extern "C" int ig_upload_contacts(ig_ctx* c, const int32_t* row, const int32_t* col, const int32_t* cnt, int64_t Z, int32_t M,
                                  int32_t rank, int32_t world)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (Z < 0 || M <= 0) return fail("ig_upload_contacts: bad sizes");
    if (world < 1 || rank < 0 || rank >= world) return fail("ig_upload_contacts: bad shard %d/%d", rank, world);
    if (c->M && c->M != M) return fail("ig_upload_contacts: M=%d does not match the sub-fragment table (%d)", M, c->M);
    c->nh_valid = false;
    c->nh_pending_slot = -1;
    free_lift_buffers(c); /* (a built ig_assembly_contacts result is of the contacts that go away now) */
    free_join_buffers(c, false); /* (and so is a built ig_join_support result) */
    std::vector<long long> rp((size_t)M + 1, 0);
    std::vector<int2> cc((size_t)Z);
    int max_count = 0;
    for (int64_t k = 0; k < Z; k++) {
        max_count = std::max(max_count, (int)cnt[k]);
        const int r = row[k], q = col[k];
        if (r < 0 || r >= M || q <= r || q >= M) return fail("ig_upload_contacts: entry %lld (%d,%d) is not strict upper triangle", (long long)k, r, q);
        if (k > 0 && (row[k - 1] > r || (row[k - 1] == r && col[k - 1] >= q)))
            return fail("ig_upload_contacts: entries must be row-major sorted and distinct (at %lld)", (long long)k);
        rp[(size_t)r + 1]++;
        cc[(size_t)k] = make_int2(q, cnt[k]);
    }
    for (int i = 0; i < M; i++) rp[(size_t)i + 1] += rp[(size_t)i];
    hipFree(c->rowptr);
    hipFree(c->cc);
    hipFree(c->crow);
    hipFree(c->tabrec);
    DALLOC(c->rowptr, (size_t)M + 1);
    DALLOC(c->cc, (size_t)Z);
    DALLOC(c->crow, (size_t)std::max<int64_t>(Z, 1));
    DALLOC(c->tabrec, (size_t)M);
    if (!c->full_const) DALLOC(c->full_const, 1);
    if (Z) HIPCK(hipMemcpy(c->crow, row, (size_t)Z * sizeof(int), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->rowptr, rp.data(), ((size_t)M + 1) * sizeof(long long), hipMemcpyHostToDevice));
    if (Z) HIPCK(hipMemcpy(c->cc, cc.data(), (size_t)Z * sizeof(int2), hipMemcpyHostToDevice));
    /* the tiled copy for the from-scratch pass (k_full_nz_tiled): counting sort of the contacts by (row block, column block) */
    hipFree(c->tiled_cc);
    hipFree(c->tile_work);
    hipFree(c->tile_hist);
    hipFree(c->tile_sig);
    hipFree(c->tile_info);
    hipFree(c->tile_dyn);
    hipFree(c->tile_dyn_list);
    hipFree(c->tile_partial);
    hipFree(c->tile_partial0);
    c->tile_partial0 = nullptr;
    c->tile_partial = nullptr;
    c->tile_info = nullptr;
    c->tile_dyn = nullptr;
    c->tile_dyn_list = nullptr;
    c->tiled_cc = nullptr;
    c->tile_work = nullptr;
    c->tile_hist = nullptr;
    c->tile_sig = nullptr;
    c->n_tile_work = 0;
    {
        const int64_t nb = ((int64_t)M + FULL_TB - 1) / FULL_TB;
        if (Z > 0 && nb <= 2048) {
            static bool s_attr = false;
            if (!s_attr) {
                HIPCK(hipFuncSetAttribute((const void*)k_full_nz_tiled, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                s_attr = true;
            }
            std::vector<int64_t> tptr((size_t)(nb * nb) + 1, 0); /* contacts per tile -> first contact of a tile */
            for (int64_t k = 0; k < Z; k++) tptr[(size_t)((row[k] / FULL_TB) * nb + col[k] / FULL_TB) + 1]++;
            for (size_t i = 1; i < tptr.size(); i++) tptr[i] += tptr[i - 1];
            /* histogram of the counts of every off-diagonal tile (a tile that turns out to hold trans pairs only is summed
             * from it, k_tile_trans); tiles with a count outside 1 .. TILE_HB-1 have none: their items are static, like the
             * diagonal tiles' */
            std::vector<int> tile_hist((size_t)(nb * nb), -1);
            std::vector<unsigned> hist;
            std::vector<TileInfo> tiles;
            {
                std::vector<char> bad((size_t)(nb * nb), 0);
                for (int64_t k = 0; k < Z; k++)
                    if (cnt[k] < 1 || cnt[k] >= TILE_HB) bad[(size_t)((row[k] / FULL_TB) * nb + col[k] / FULL_TB)] = 1;
                for (int64_t bi = 0; bi < nb; bi++)
                    for (int64_t bj = bi + 1; bj < nb; bj++) {
                        const size_t t = (size_t)(bi * nb + bj);
                        if (!bad[t] && tptr[t + 1] > tptr[t] && tptr[t + 1] - tptr[t] < (1LL << 31)) {
                            tile_hist[t] = (int)tiles.size();
                            tiles.push_back(TileInfo{(int)bi, (int)bj, 0, 0});
                        }
                    }
                hist.assign(std::max<size_t>(tiles.size(), 1) * TILE_HB, 0u);
                for (int64_t k = 0; k < Z; k++) {
                    const int h = tile_hist[(size_t)((row[k] / FULL_TB) * nb + col[k] / FULL_TB)];
                    if (h >= 0) hist[(size_t)h * TILE_HB + cnt[k]]++;
                }
            }
            /* work items: the static ones first (k_full_nz_tiled's grid), then those of the tiles with a histogram */
            std::vector<TileWork> work;
            for (int pass = 0; pass < 2; pass++) {
                for (int64_t bi = 0; bi < nb; bi++)
                    for (int64_t bj = bi; bj < nb; bj++) {
                        const int64_t b = tptr[(size_t)(bi * nb + bj)], e = tptr[(size_t)(bi * nb + bj) + 1];
                        const int h = tile_hist[(size_t)(bi * nb + bj)];
                        if ((h >= 0) != (pass == 1)) continue;
                        if (h >= 0) tiles[(size_t)h].first_item = (int)work.size();
                        const size_t first = work.size();
                        for (int64_t o = b; o < e; o += FULL_CHUNK)
                            work.push_back(TileWork{(long long)o, (int)std::min<int64_t>(FULL_CHUNK, e - o), (int)bi, (int)bj, 0});
                        for (size_t q = first; q < work.size(); q++) work[q].pad = (int)(work.size() - 1 - q); /* items of this tile behind this one */
                        if (h >= 0) tiles[(size_t)h].n_items = (int)work.size() - tiles[(size_t)h].first_item;
                    }
                if (pass == 0) c->n_tile_static = (int)work.size();
            }
            std::vector<uint2> tc((size_t)Z);
            std::vector<int64_t> cur(tptr.begin(), tptr.end() - 1);
            for (int64_t k = 0; k < Z; k++) {
                const int64_t t = (row[k] / FULL_TB) * nb + col[k] / FULL_TB;
                tc[(size_t)cur[(size_t)t]++] = make_uint2((unsigned)(row[k] % FULL_TB) | ((unsigned)(col[k] % FULL_TB) << 11), (unsigned)cnt[k]);
            }
            DALLOC(c->tiled_cc, (size_t)Z);
            DALLOC(c->tile_work, work.size());
            DALLOC(c->tile_hist, hist.size());
            DALLOC(c->tile_sig, (size_t)nb * (SIG_WORDS + SIG_FOLD));
            DALLOC(c->tile_info, std::max<size_t>(tiles.size(), 1));
            DALLOC(c->tile_dyn, 4);
            DALLOC(c->tile_partial, 2 * ((tiles.size() + TILE_TRANS_THREADS / 64 - 1) / (TILE_TRANS_THREADS / 64) + 1));
            DALLOC(c->tile_partial0, 2 * ((tiles.size() + TILE_TRANS_THREADS / 64 - 1) / (TILE_TRANS_THREADS / 64) + 1));
            DALLOC(c->tile_dyn_list, std::max<size_t>(work.size() - (size_t)c->n_tile_static, 1));
            HIPCK(hipMemcpy(c->tiled_cc, tc.data(), (size_t)Z * sizeof(uint2), hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(c->tile_work, work.data(), work.size() * sizeof(TileWork), hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(c->tile_hist, hist.data(), hist.size() * sizeof(unsigned), hipMemcpyHostToDevice));
            if (!tiles.empty()) HIPCK(hipMemcpy(c->tile_info, tiles.data(), tiles.size() * sizeof(TileInfo), hipMemcpyHostToDevice));
            c->n_tile_info = (int)tiles.size();
            c->n_tile_work = (int)work.size();
        }
    }
    c->Z = Z;
    c->M = M;
    c->max_count = max_count;
    c->rank = rank;
    c->world = world;
    c->have_contacts = true;
    return 0;
}

extern "C" int ig_upload_subfrag_table(ig_ctx* c, const float* xyzw, int32_t M)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (M <= 0) return fail("ig_upload_subfrag_table: M <= 0");
    if (c->M && c->M != M) return fail("ig_upload_subfrag_table: M=%d does not match the contacts (%d)", M, c->M);
    std::vector<SubTab> t((size_t)M);
    for (int s = 0; s < M; s++) {
        t[s].parent = (int)xyzw[4 * (size_t)s];
        t[s].wat = xyzw[4 * (size_t)s + 1];
        t[s].cri = xyzw[4 * (size_t)s + 2];
        t[s].w = (int)xyzw[4 * (size_t)s + 3];
        if (s > 0 && (t[s].parent < t[s - 1].parent || (t[s].parent == t[s - 1].parent && t[s].w != t[s - 1].w + 1)))
            return fail("ig_upload_subfrag_table: sub-fragments of a bin must be contiguous and ordered (at %d)", s);
    }
    hipFree(c->sub_tab);
    DALLOC(c->sub_tab, (size_t)M);
    HIPCK(hipMemcpy(c->sub_tab, t.data(), (size_t)M * sizeof(SubTab), hipMemcpyHostToDevice));
    hipFree(c->tab.dist);
    hipFree(c->tab_prev.dist);
    for (Tables* tb : {&c->tab, &c->tab_prev}) {
        int* blk;
        DALLOC(blk, 6 * (size_t)M + 2);
        tb->dist = (float*)blk;
        tb->stot = (float*)(blk + (size_t)M);
        tb->len = blk + 2 * (size_t)M;
        tb->cp = (int2*)(blk + 4 * (size_t)M + ((4 * (size_t)M) & 1)); /* keep the int2 array 8-byte aligned */
    }
    hipFree(c->prev_touched);
    DALLOC(c->prev_touched, (size_t)M);
    hipFree(c->touched_bits);
    DALLOC(c->touched_bits, 2 * ((size_t)(M + 31) / 32 + 1));
    HIPCK(memset_now(c->touched_bits, 0, 2 * ((size_t)(M + 31) / 32 + 1) * sizeof(unsigned)));
    c->M = M;
    c->have_sub = true;
    return 0;
}

static int launch_recompute(ig_ctx* c);

/* the incremental genome distance of k_commit_batch evaluates every credit a move can change exactly once; its rule for
 * telling who evaluates a fragment reached through several links needs the initial prev / next to be mutually inverse
 * (true of every genome made of contigs; an arbitrary pair of arrays takes the one-move path, which recounts all credits) */
static bool links_inverse(const int32_t* ip, const int32_t* in, size_t n)
{
    for (size_t f = 0; f < n; f++) {
        const int p = ip[f], q = in[f];
        if (p < -1 || q < -1 || p >= (int)n || q >= (int)n) return false;
        if (p >= 0 && (in[p] != (int)f || p == (int)f)) return false;
        if (q >= 0 && (ip[q] != (int)f || q == (int)f)) return false;
        if (p >= 0 && p == q) return false;
    }
    return true;
}

extern "C" int ig_upload_state(ig_ctx* c, const int32_t* soa, int32_t N)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (N <= 0) return fail("ig_upload_state: N <= 0");
    if (!c->have_sub) return fail("ig_upload_state: upload the sub-fragment table first");
    c->nuis_spec = c->spec_valid = false;
    const size_t n = N;
    std::vector<int> host(17 * n);
    /* soa member order (KA:40-58): 0 pos 1 sub_pos 2 id_c 3 start_bp 4 len_bp 5 sub_len 6 circ 7 id 8 prev 9 next
     * 10 l_cont 11 sub_l_cont 12 l_cont_bp 13 ori 14 rep 15 activ 16 id_d */
    static const int dyn_src[NDYN] = {0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13};
    for (int k = 0; k < NDYN; k++) memcpy(&host[k * n], soa + dyn_src[k] * n, n * sizeof(int));
    memcpy(&host[11 * n], soa + 4 * n, n * sizeof(int));  /* len_bp */
    memcpy(&host[12 * n], soa + 5 * n, n * sizeof(int));  /* sub_len */
    memcpy(&host[14 * n], soa + 14 * n, n * sizeof(int)); /* rep */
    memcpy(&host[15 * n], soa + 15 * n, n * sizeof(int)); /* activ */
    memcpy(&host[16 * n], soa + 16 * n, n * sizeof(int)); /* id_d */
    /* first sub-fragment of each bin + consistency with the table */
    std::vector<SubTab> t((size_t)c->M);
    HIPCK(hipMemcpy(t.data(), c->sub_tab, (size_t)c->M * sizeof(SubTab), hipMemcpyDeviceToHost));
    long long acc = 0;
    for (size_t f = 0; f < n; f++) {
        host[13 * n + f] = (int)acc;
        const int sl = soa[5 * n + f];
        if (sl < 1 || acc + sl > c->M) return fail("ig_upload_state: sub_len of bin %zu inconsistent with the sub-fragment table", f);
        for (int w = 0; w < sl; w++)
            if (t[(size_t)acc + w].parent != (int)f || t[(size_t)acc + w].w != w)
                return fail("ig_upload_state: sub-fragment %lld is not (bin %zu, index %d)", acc + w, f, w);
        acc += sl;
        if (soa[15 * n + f] != 1) return fail("ig_upload_state: inactive fragments are not supported (dead in the reference)");
    }
    if (acc != c->M) return fail("ig_upload_state: bins cover %lld sub-fragments, table has %d", acc, c->M);
    /* internal contig ids: any injective relabelling works; keep the caller's, they are >= 0 */
    int max_c = 0;
    for (size_t f = 0; f < n; f++) {
        if (soa[2 * n + f] < 0) return fail("ig_upload_state: negative contig id");
        max_c = std::max(max_c, soa[2 * n + f]);
    }
    hipFree(c->st_block);
    DALLOC(c->st_block, 17 * n);
    HIPCK(hipMemcpy(c->st_block, host.data(), 17 * n * sizeof(int), hipMemcpyHostToDevice));
    int** sp = (int**)&c->st;
    for (int k = 0; k < 17; k++) sp[k] = c->st_block + k * n;
    const bool size_changed = (c->N != N);
    c->N = N;
    if (size_changed || !c->have_init) { /* default initial genome for the distance = this state (CL:269-276) */
        hipFree(c->init_prev);
        hipFree(c->init_next);
        hipFree(c->orientable);
        hipFree(c->black);
        DALLOC(c->init_prev, n);
        DALLOC(c->init_next, n);
        DALLOC(c->orientable, n);
        DALLOC(c->black, n);
        std::vector<int> orient(n);
        for (size_t f = 0; f < n; f++) orient[f] = soa[5 * n + f] > 1;
        HIPCK(hipMemcpy(c->init_prev, soa + 8 * n, n * sizeof(int), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(c->init_next, soa + 9 * n, n * sizeof(int), hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(c->orientable, orient.data(), n * sizeof(int), hipMemcpyHostToDevice));
        HIPCK(memset_now(c->black, 0, n));
        c->have_init = true;
        c->init_links_inverse = links_inverse(soa + 8 * n, soa + 9 * n, n);
    }
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    hg.N = N;
    hg.M = c->M;
    hg.next_cid = max_c + 1;
    hg.n_tot_pxl = (double)c->M * ((double)c->M - 1.0) / 2.0; /* CL:366 */
    for (int i = 0; i < 12; i++) hg.valid_insert[i] = 0; /* CL:421 */
    hg.error = 0;
    HIPCK(hipMemcpy(c->glob, &hg, sizeof hg, hipMemcpyHostToDevice));
    c->have_state = true;
    if (ensure_move_buffers(c, 8)) return -1;
    return launch_recompute(c);
}

/* tables, head count, genome-distance credits and (when parameters are known) the exact
 * likelihood sums of the current state */
static int launch_recompute(ig_ctx* c)
{
    c->nh_valid = false; /* (the histogram of the screened nuisance pass: rebuilt by the next run) */
    c->nh_pending_slot = -1;
    if (!c->have_state || !c->have_sub) return 0;
    const int N = c->N, M = c->M;
    hipLaunchKernelGGL(k_fill_tables, dim3((M + 255) / 256), dim3(256), 0, c->stream, c->st, c->sub_tab, c->tab, M);
    HIPCK(hipMemcpyAsync(c->tab_prev.dist, c->tab.dist, (6 * (size_t)M + 2) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    long long* scratch = c->scratch8; /* persistent: an allocation per call costs more than the small kernels */
    HIPCK(hipMemsetAsync(scratch, 0, 8 * sizeof(long long), c->stream));
    int* heads = (int*)(scratch + 6);
    HIPCK(hipMemsetAsync(&c->glob->max_L, 0, 2 * sizeof(int), c->stream)); /* max_L, max_SL: recounted */
    hipLaunchKernelGGL(k_count_heads, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->st, N, heads, c->glob);
    HIPCK(hipMemsetAsync(&c->glob->credit2_acc, 0, sizeof(long long), c->stream));
    hipLaunchKernelGGL(k_post, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->st, c->init_prev, c->init_next, c->orientable,
                       c->black, c->glob, N);
    if (c->have_params && c->have_contacts) {
        launch_full_nz(c, c->tab, 0, scratch, PzTab{c->pz_tab, c->pz_n});
        hipLaunchKernelGGL(k_full_zero, dim3(128), dim3(256), 0, c->stream, c->tab, c->glob, 0, M, scratch + 2);
    }
    long long h[8];
    HIPCK(hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    ig_acc_normalize((int64_t*)&h[0], (int64_t*)&h[1]);
    ig_acc_normalize((int64_t*)&h[2], (int64_t*)&h[3]);
    hg.nz_hi = h[0];
    hg.nz_lo = h[1];
    hg.z_hi = h[2];
    hg.z_lo = h[3];
    hg.n_intra = h[4];
    hg.n_contigs = ((int*)&h[6])[0];
    c->max_L = hg.max_L;
    c->max_SL = hg.max_SL;
    hg.credit2 = hg.credit2_acc;
    hg.credit2_acc = 0;
    hg.n_prev_touched = 0;
    HIPCK(hipMemcpy(c->glob, &hg, sizeof hg, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int ig_set_params(ig_ctx* c, const float p[8], float mean_subfrag_kb, int which)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (which != 0 && which != 1) return fail("ig_set_params: which must be 0 or 1");
    if (which == 0) c->nuis_spec = c->spec_valid = false; /* moves scored ahead (ig_nuis_step_begin) were scored under the old set */
    HIPCK(hipStreamSynchronize(c->stream));
    ig_params hp = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
    if (which == 0) c->par_model = hp;
    HIPCK(hipMemcpy(&c->glob->par[which], &hp, sizeof hp, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(&c->glob->mean_kb, &mean_subfrag_kb, sizeof(float), hipMemcpyHostToDevice));
    {
        /* P_z table of this parameter set; length: first rank distance whose s_z reaches d_max (+1), capped */
        float*& tab = which == 0 ? c->pz_tab : c->pz_tab1;
        int& n = which == 0 ? c->pz_n : c->pz_n1;
        if (!tab) DALLOC(tab, PZ_MAX);
        double need = (mean_subfrag_kb > 0) ? (double)p[5] / (double)mean_subfrag_kb + 2.0 : 0.0;
        n = (need > 0 && need < (double)PZ_MAX) ? (int)need : ((need >= (double)PZ_MAX) ? PZ_MAX : 0);
        if (n > 0) hipLaunchKernelGGL(k_build_pz, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->glob, tab, n, which);
        if (which == 0) { /* the constants k_score_list stages */
            if (!c->score_const) DALLOC(c->score_const, 1);
            hipLaunchKernelGGL(k_build_score_const, dim3((LDS_PZ + 2 + 255) / 256), dim3(256), 0, c->stream, c->glob, PzTab{tab, n}, c->lgf_tab,
                               c->score_const, 0);
            if (!c->screen_const) DALLOC(c->screen_const, 1);
            hipLaunchKernelGGL(k_build_screen_const, dim3((LDS_PZ + 2 + 255) / 256), dim3(256), 0, c->stream, c->glob, PzTab{tab, n}, c->screen_const);
        }
    }
    if (which == 0) {
        c->have_params = true;
        return launch_recompute(c); /* the maintained exact sums depend on param_simu */
    }
    return 0;
}

extern "C" int ig_set_insert_config(ig_ctx* c, const int32_t list_bounds[IG_N_INSERT_BLOCKS], int32_t max_bounds_insert)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(c->glob->list_bounds, list_bounds, 6 * sizeof(int), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(&c->glob->slice_nb, &max_bounds_insert, sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int ig_set_initial_genome(ig_ctx* c, const int32_t* ip, const int32_t* in, const int32_t* orientable,
                                     const int32_t* blacklisted, int32_t nb)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->have_state) return fail("ig_set_initial_genome: upload the state first");
    const size_t n = c->N;
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(c->init_prev, ip, n * sizeof(int), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->init_next, in, n * sizeof(int), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(c->orientable, orientable, n * sizeof(int), hipMemcpyHostToDevice));
    std::vector<unsigned char> b(n, 0);
    for (int i = 0; i < nb; i++) {
        if (blacklisted[i] < 0 || (size_t)blacklisted[i] >= n) return fail("ig_set_initial_genome: blacklisted id out of range");
        b[blacklisted[i]] = 1;
    }
    int cnt = 0;
    for (size_t i = 0; i < n; i++) cnt += b[i];
    HIPCK(hipMemcpy(c->black, b.data(), n, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(&c->glob->n_black, &cnt, sizeof(int), hipMemcpyHostToDevice));
    c->init_links_inverse = links_inverse(ip, in, n);
    return launch_recompute(c);
}

/* canonical contig numbering of modify_gl_cuda_buffer (CL:2715-2881): contigs enumerated by
 * ascending index of their pos==0 fragment (the order an in-order select_uniq_id_c produces,
 * KA:357-406), stable sort by length descending (CL:69-77), id = (n-1) - rank (KA:4689-4692). */
static void canonical_ids(const int* pos, const int* cid, const int* L, size_t n, std::vector<int>& out, int* n_contigs)
{
    std::vector<int> heads;
    for (size_t f = 0; f < n; f++)
        if (pos[f] == 0) heads.push_back((int)f);
    std::vector<int> order(heads.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return L[heads[a]] > L[heads[b]]; });
    int max_c = 0;
    for (size_t f = 0; f < n; f++) max_c = std::max(max_c, cid[f]);
    std::vector<int> map((size_t)max_c + 1, -1);
    const int nc = (int)heads.size();
    for (int r = 0; r < nc; r++) map[cid[heads[order[r]]]] = (nc - 1) - r;
    out.resize(n);
    for (size_t f = 0; f < n; f++) out[f] = map[cid[f]];
    *n_contigs = nc;
}

extern "C" int ig_download_state(ig_ctx* c, int32_t* soa)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->have_state) return fail("ig_download_state: no state");
    const size_t n = c->N;
    HIPCK(hipStreamSynchronize(c->stream));
    std::vector<int> host(17 * n);
    HIPCK(hipMemcpy(host.data(), c->st_block, 17 * n * sizeof(int), hipMemcpyDeviceToHost));
    static const int dyn_src[NDYN] = {0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13};
    for (int k = 0; k < NDYN; k++) memcpy(soa + dyn_src[k] * n, &host[k * n], n * sizeof(int));
    memcpy(soa + 4 * n, &host[11 * n], n * sizeof(int));
    memcpy(soa + 5 * n, &host[12 * n], n * sizeof(int));
    memcpy(soa + 14 * n, &host[14 * n], n * sizeof(int));
    memcpy(soa + 15 * n, &host[15 * n], n * sizeof(int));
    memcpy(soa + 16 * n, &host[16 * n], n * sizeof(int));
    for (size_t f = 0; f < n; f++) soa[7 * n + f] = (int)f;
    std::vector<int> ids;
    int nc;
    canonical_ids(&host[0], &host[2 * n], &host[7 * n], n, ids, &nc);
    memcpy(soa + 2 * n, ids.data(), n * sizeof(int));
    return 0;
}

extern "C" int ig_renumber_contigs(ig_ctx* c, int32_t* n_contigs, float* mean_len, int32_t* max_id)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    int nc;
    HIPCK(hipMemcpy(&nc, &c->glob->n_contigs, sizeof(int), hipMemcpyDeviceToHost));
    if (n_contigs) *n_contigs = nc;
    if (mean_len) *mean_len = (float)c->N / (float)nc;
    if (max_id) *max_id = nc - 1;
    return 0;
}

extern "C" int ig_bomb(ig_ctx* c, const int32_t* shuffle)
{
    IG_JOIN(c);
    (void)shuffle; /* explode_genome writes id_c = shuffle[i] (KA:419); the renumbering that follows (CL:1948) erases it */
    HIPCK(hipSetDevice(c->device));
    if (!c->have_state) return fail("ig_bomb: no state");
    c->nuis_spec = c->spec_valid = false;
    hipLaunchKernelGGL(k_explode, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->st, c->N);
    int next = c->N;
    HIPCK(hipMemcpyAsync(&c->glob->next_cid, &next, sizeof(int), hipMemcpyHostToDevice, c->stream));
    return launch_recompute(c);
}

extern "C" int ig_genome_distance(ig_ctx* c, double* d)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    const double norm = 3.0 * (double)(hg.N - hg.n_black);
    *d = (norm - 0.5 * (double)hg.credit2) / norm;
    return 0;
}

extern "C" int ig_get_valid_insert(ig_ctx* c, int32_t out12[12])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(out12, c->glob->valid_insert, 12 * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

/* nz and z of the five normalised limbs {nz hi, nz lo, z hi, z lo, intra pairs} (either may be NULL): what ig_full_likelihood returns
 * and what ig_edit_score returns for an edited genome (ig_host_edit.inc) -- one statement, so the two are the same doubles */
static void likelihood_of_limbs(const long long h[5], double n_tot_pxl, float v_inter, double* nz, double* z)
{
    if (nz) *nz = ig_acc_to_double(h[0], h[1]);
    if (z) { /* CL:755-759 with the float log_e of the kernels replaced by the host's double constant */
        const double log_e = 0.43429448190325182;
        const double val_intra = ig_acc_to_double(h[2], h[3]) * log_e;
        const double val_inter = log_e * (n_tot_pxl - (double)h[4]) * -1.0 * (double)v_inter;
        *z = val_intra + val_inter;
    }
}

extern "C" int ig_full_likelihood(ig_ctx* c, int which, int use_prev, double* nz, double* z, int64_t* limbs5)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->have_contacts || !c->have_state || !c->have_params) return fail("ig_full_likelihood: contacts, state and parameters are required");
    if (which != 0 && which != 1) return fail("ig_full_likelihood: which must be 0 or 1");
    long long* scratch = c->scratch8; /* persistent: an allocation per call costs more than the small kernels */
    HIPCK(hipMemsetAsync(scratch, 0, 8 * sizeof(long long), c->stream));
    Tables& t = use_prev ? c->tab_prev : c->tab;
    /* which == 1 before any ig_set_params(.., 1): no table yet, every P_z is evaluated directly */
    const PzTab pz = which == 0 ? PzTab{c->pz_tab, c->pz_n} : PzTab{c->pz_tab1, c->pz_tab1 ? c->pz_n1 : 0};
    if (!launch_full_nz(c, t, which, scratch, pz, nullptr, scratch + 2))
        hipLaunchKernelGGL(k_full_zero, dim3(128), dim3(256), 0, c->stream, t, c->glob, which, c->M, scratch + 2);
    long long h[8];
    HIPCK(hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    ig_acc_normalize((int64_t*)&h[0], (int64_t*)&h[1]);
    ig_acc_normalize((int64_t*)&h[2], (int64_t*)&h[3]);
    double n_tot_pxl;
    float v_inter;
    const int vi_bits = (int)h[7];
    memcpy(&n_tot_pxl, &h[5], sizeof n_tot_pxl); /* k_full_zero: n_tot_pxl and v_inter of the parameter set */
    memcpy(&v_inter, &vi_bits, sizeof v_inter);
    likelihood_of_limbs(h, n_tot_pxl, v_inter, nz, z);
    if (limbs5)
        for (int i = 0; i < 5; i++) limbs5[i] = h[i];
    return 0;
}
