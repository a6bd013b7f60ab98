/* ig_host_nuis.inc -- part of ig_hip.hip (one translation unit; included there in order): the nuisance step next to its move: one pair per call, runs of pairs with the moves scored ahead, the screened Metropolis test (histogram tier, float pass, exact pass), promotion of an accepted step, chains of pairs decided on the device. */

/* ---- a move and the nuisance step that follows it, in flight together (instagraal.py:217-262 for cycles > 4) ----------
 * step_nuisance_parameters (CL:2961-3051) evaluates the full likelihood under its test parameters on the coordinates of the
 * state BEFORE the move that was just applied (quirk Q12) and needs nothing else from that move but its score: the pass
 * over all contacts does not have to wait for the move.  ig_nuis_begin enqueues the move (score + apply, library stream)
 * and, on a second stream behind the move's k_gather (after which tab_prev is that earlier state), the full pass under
 * p_test; ig_nuis_end waits for both; ig_nuis_accept makes the test parameters the model's. */
/* tab_prev := the state before the move about to be scored (what k_gather does first thing; here ahead of it, so that the
 * nuisance pass can start next to the move instead of behind its launches) */
__global__ void k_catch_up(Tables tab, Tables tab_prev, const int* __restrict__ prev_touched, const Glob* g)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < g->n_prev_touched; i += gridDim.x * blockDim.x) {
        const int s = prev_touched[i];
        tab_prev.dist[s] = tab.dist[s];
        tab_prev.stot[s] = tab.stot[s];
        tab_prev.cp[s] = tab.cp[s];
        tab_prev.len[s] = tab.len[s];
    }
}

/* pinned and mapped: the kernels write a step's results there themselves and raise a flag (no copy, no stream synchronisation) */
static int ensure_host_nuis(ig_ctx* c)
{
    if (c->host_nuis) return 0;
    c->host_nuis = (NuisHost*)mapped_block(sizeof(NuisHost), (void**)&c->host_nuis_dev, false);
    if (c->host_nuis) return 0;
    HIPCK(hipHostMalloc((void**)&c->host_nuis, sizeof(NuisHost), hipHostMallocDefault));
    memset(c->host_nuis, 0, sizeof(NuisHost));
    return 0;
}

/* spin until *flag == seq (written by a kernel into mapped host memory) or `stream` has drained; true: the flag is there */
static bool wait_host_flag(volatile int* flag, int seq, hipStream_t stream)
{
    for (unsigned spin = 0;; spin++) {
        if (*flag == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return true;
        }
        if ((spin & 0xfff) == 0xfff && hipStreamQuery(stream) != hipErrorNotReady) return *flag == seq;
    }
}

/* ---- the Metropolis test from a screened pass (ig_kernels_nuis.cuh) ------------------------------------------------------
 * IG_NUIS_SCREEN=0: every step through the exact pass, as before; IG_NUIS_SCREEN_VERIFY=1: both, the bound checked on the host */
static int g_nuis_screen = -1, g_nuis_screen_verify = 0, g_nuis_hist_trace = 0;
static int g_nuis_hist = -1; /* tier 0 of the screened pass: ig_set_nuis_hist / IG_NUIS_HIST (0: off, 1: where its cost model says, 2: always) */
static int g_nuis_chain = -1; /* chains of pairs decided on the device: ig_set_nuis_chain / IG_NUIS_CHAIN (default 1) */
static int g_nuis_w = -1;    /* moves scored ahead per launch in a run of ig_nuis_step_begin: env IG_NUIS_W, ig_set_nuis_width; 0: follow the run lengths */
static void nuis_latch_env()
{
    if (g_nuis_hist < 0) g_nuis_hist = getenv("IG_NUIS_HIST") ? atoi(getenv("IG_NUIS_HIST")) : 1;
    if (g_nuis_w < 0) g_nuis_w = getenv("IG_NUIS_W") ? std::max(0, atoi(getenv("IG_NUIS_W"))) : 0;
    if (g_nuis_chain < 0) g_nuis_chain = getenv("IG_NUIS_CHAIN") ? atoi(getenv("IG_NUIS_CHAIN")) : 1;
    if (g_nuis_screen < 0) g_nuis_screen = getenv("IG_NUIS_SCREEN") ? atoi(getenv("IG_NUIS_SCREEN")) : 1;
    g_nuis_screen_verify = getenv("IG_NUIS_SCREEN_VERIFY") ? atoi(getenv("IG_NUIS_SCREEN_VERIFY")) : 0; /* per run: a test toggles it */
    g_nuis_hist_trace = getenv("IG_NUIS_HIST_TRACE") ? atoi(getenv("IG_NUIS_HIST_TRACE")) : 0;
    g_nuis_async = getenv("IG_NUIS_ASYNC") ? atoi(getenv("IG_NUIS_ASYNC")) : 1;
}
static bool nuis_screen_usable(ig_ctx* c)
{
    /* (the environment is read on the caller's thread, where a run begins -- nuis_latch_env: this function also runs on the helper
     * thread, and getenv next to a setenv of the interpreter's thread is undefined) */
    return (g_nuis_screen || g_nuis_screen_verify) && c->nuis_spec && c->host_nuis_dev && c->tiled_cc && c->n_tile_work > 0 &&
           c->score_const && c->screen_const && c->pz_tab && g_full_hist != 0;
}
extern "C" int ig_set_nuis_screen(int on)
{
    g_nuis_screen = on ? 1 : 0;
    return 0;
}

/* the exact tiles kernel over the list the step's k_tile_trans left (tables, signatures, constants of the test set are in place) */
static void launch_nuis_exact_tiles(ig_ctx* c, hipStream_t s3, long long* out = nullptr, bool publish = true)
{
    if (!out) out = c->scratch_nuis;
    const int s_grid = 512;
    const int per = TILE_TRANS_THREADS / 64;
    const int n_trans = (c->n_tile_info + per - 1) / per;
    const int grid = std::min(c->n_tile_work, s_grid);
    hipLaunchKernelGGL(k_full_nz_tiled, dim3(grid), dim3(FULL_TILED_THREADS), sizeof(FullTiledLds), s3, c->tile_work, c->tiled_cc, c->tabrec,
                       c->tab_prev.len, c->full_const, c->lgf_tab, c->M, c->pz_n1, out, c->n_tile_static, (TileDyn*)c->tile_dyn,
                       c->tile_dyn_list, (long long*)nullptr, publish ? c->host_nuis_dev : (NuisHost*)nullptr, publish ? ++c->sums_seq : 0, c->tile_partial,
                       n_trans);
    if (publish) c->nuis_pub_sums = true;
}

/* tier 0 of the screened pass (ig_kernels_nuis.cuh): the histogram of the cis contacts' distances.  IG_NUIS_HIST=0: off */
static bool nuis_hist_usable(ig_ctx* c)
{
    if (g_nuis_hist < 0) g_nuis_hist = 1; /* (IG_NUIS_HIST: nuis_latch_env) */
    if (!g_nuis_hist || !nuis_screen_usable(c)) return false;
    if (g_nuis_hist >= 2) return true; /* (2: whatever the cost model says -- tests) */
    /* The histogram pays where the pass over the contacts is long and the moves are local.  Per step it costs its evaluation
     * (~16 us) plus, for the share p of the moves that change the genome, the walk over the contacts inside the move's two contigs
     * -- about 2 Z / n_contigs of them, 10 atomics each at ~24 G/s (profiles/r03_microbench.txt); the pass over the contacts costs
     * ~20 us of launches + the cis tiles' 8 bytes per contact at ~5 TB/s.  Few long contigs (the late stage of an assembly: 4
     * contigs of 1 000 bins, 58 % of the moves change the genome) turn the balance: 3.0 k (move + step)/s with the histogram
     * there, 3.9 k without.  With hysteresis; a histogram that is switched off is dropped (the walks stop) and rebuilt when it
     * comes back. */
    const double Z = (double)c->Z, nc = (double)std::max(c->n_contigs_seen, 1), p = c->nh_p_changed;
    /* (the pass over the contacts is void where a table is longer than its staged part and a contig longer than that -- it reads P_z
     * by rank distance from LDS only -- and the exact pass, ~2.5 x the float one, runs instead; the histogram keeps every rank distance) */
    const bool t1_void = std::max(c->pz_n, c->pz_n1) > LDS_PZ && c->max_SL > LDS_PZ;
    const double t0 = 16.0 + p * (2.0 * Z / nc) * 10.0 / 24e3, t1 = 20.0 + Z * 8.0 * 0.4 / 5e6 * (t1_void ? 2.5 : 1.0);
    if (c->n_contigs_seen <= 0) return c->nh_policy_on; /* (no batch decided yet) */
    if (c->nh_policy_on ? t0 > 1.25 * t1 : t0 < 0.8 * t1) {
        c->nh_policy_on = !c->nh_policy_on;
        if (!c->nh_policy_on) {
            c->nh_valid = false;
            c->nh_pending_slot = -1;
        }
    }
    return c->nh_policy_on;
}
extern "C" int ig_set_nuis_hist(int on)
{
    g_nuis_hist = on < 0 ? 0 : std::min(on, 2);
    return 0;
}
static int ensure_nuis_hist(ig_ctx* c)
{
    const int dh_n = std::max(c->M, LDS_PZ); /* a rank distance is below the number of sub-fragments */
    if (c->nh.bins && c->nh.dh_n == dh_n) return 0;
    if (c->nh.bins) {
        hipFree(c->nh.bins);
        hipFree(c->nh.dh);
        hipFree(c->nh.misc);
        hipFree(c->scratch_hist);
        c->nh = NuisHist{nullptr, nullptr, nullptr, 0};
        c->scratch_hist = nullptr;
    }
    DALLOC(c->nh.bins, (size_t)NH_NB * 4);
    DALLOC(c->nh.dh, (size_t)dh_n + 1);
    DALLOC(c->nh.misc, NH_MISC);
    c->nh.dh_n = dh_n;
    DALLOC(c->scratch_hist, 16);
    HIPCK(memset_now(c->scratch_hist, 0, 16 * sizeof(long long)));
    c->nh_valid = false;
    return 0;
}
/* the last move of the run is not in the histogram yet (a step is evaluated on the state BEFORE its move): walk it in now -- before
 * anything replaces what the walk reads: the move's slot in the batch buffers, and tab_prev as of before the move */
static int nh_flush_pending(ig_ctx* c)
{
    const int w = c->nh_pending_slot;
    c->nh_pending_slot = -1;
    if (w < 0 || !c->nh_valid || !c->nh.bins) return 0;
    const int s_blocks = 128;
    hipLaunchKernelGGL(k_hist_walk, dim3(s_blocks), dim3(256), 0, c->stream3, c->rowptr, c->cc, c->tab_prev, c->glob, c->mb, w, c->nh);
    HIPCK(hipEventRecord(c->ev_walk, c->stream3));
    HIPCK(hipStreamWaitEvent(c->stream, c->ev_walk, 0));
    c->nhs[6] += 1.0;
    return 0;
}

/* what every tier of a step's screened pass needs first: the test set's tables and constants, tab_prev caught up (fuse_catch) and
 * packed, the scratch words cleared (k_nuis_prepare) */
static int launch_nuis_prepare(ig_ctx* c, const ig_params& hp, float mean_kb, hipStream_t s3, bool fuse_catch)
{
    if (!c->diff_const) {
        DALLOC(c->diff_const, 1);
        DALLOC(c->scratch_diff, 8);
        HIPCK(hipFuncSetAttribute((const void*)k_full_diff_tiled<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(DiffLds)));
        HIPCK(hipFuncSetAttribute((const void*)k_full_diff_tiled<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(DiffLds)));
    }
    const Tables& t = c->tab_prev;
    const int n_pack = (c->M + FULL_TB - 1) / FULL_TB;
    const int n_const = (std::max(std::max(c->pz_n1, LDS_PZ + 2), std::max((int)IG_TAB_SIZE, LDS_LGF)) + 255) / 256;
    hipLaunchKernelGGL(k_nuis_prepare, dim3(n_pack + n_const), dim3(256), 0, s3, c->glob, 1, hp, mean_kb, c->pz_tab1, c->pz_n1, c->lgf_tab, c->full_const,
                       c->scratch_nuis, t, c->M, c->tabrec, c->tile_sig, FULL_TB, c->tile_dyn, n_pack, c->score_const, c->pz_n, c->diff_const,
                       c->scratch_diff, c->screen_const, fuse_catch ? c->tab : Tables{nullptr, nullptr, nullptr, nullptr}, c->prev_touched);
    /* the library stream's next kernels replace what the catch-up reads: they wait for it (not for the pass behind it) */
    if (fuse_catch) {
        HIPCK(hipEventRecord(c->ev_main, s3));
        HIPCK(hipStreamWaitEvent(c->stream, c->ev_main, 0));
    }
    c->nuis_tiles_listed = false;
    return 0;
}

/* the list of the tiles whose contacts a pass has to read, the all-trans tiles' histogram sums under both sets (k_tile_trans);
 * with_zero: the zero-pixel sum of the test set in the same launch (else: someone else's job -- the histogram tier's launch) */
static void launch_nuis_tile_list(ig_ctx* c, hipStream_t s3, bool with_zero)
{
    const int per = TILE_TRANS_THREADS / 64;
    const int n_trans = (c->n_tile_info + per - 1) / per, n_zero = with_zero ? std::min(256, std::max(32, c->M / 4096)) : 0;
    if (n_trans + n_zero > 0) /* (a matrix of a single tile has no off-diagonal ones to list) */
        hipLaunchKernelGGL(k_tile_trans, dim3(n_trans + n_zero), dim3(TILE_TRANS_THREADS), 0, s3, c->tile_info, c->n_tile_info, c->tile_sig, c->tile_hist,
                           c->full_const, (TileDyn*)c->tile_dyn, c->tile_dyn_list, 1, c->tile_partial, n_trans, c->tab_prev, c->glob, 1, c->M,
                           c->scratch_nuis + 2, c->score_const, c->tile_partial0);
    c->nuis_tiles_listed = true;
}

/* tier 1: the float pass over the contacts (k_full_diff_tiled) behind the tile list */
static int launch_nuis_diff(ig_ctx* c, const ig_params& hp, hipStream_t s3, bool with_zero)
{
    launch_nuis_tile_list(c, s3, with_zero);
    const int per = TILE_TRANS_THREADS / 64;
    const int n_trans = (c->n_tile_info + per - 1) / per;
    /* two workgroups per CU less two: the one-wave kernels of the move next to the pass (decide, commit) find a SIMD with registers
     * to spare at once (the stream workgroups take all 512 VGPRs of a SIMD between them).  (Measured and dropped: k_tile_trans's
     * blocks as the head of this kernel's grid, the stream workgroups waiting for them in front of the list: 95 - 112 us instead of
     * 11 + 68 - 84 -- 400 head blocks with this kernel's footprint hold the machine before the first contact is read.) */
    const int s_grid = 510;
    const int s_grid_side = 256;
    const int grid = std::min(c->n_tile_work, c->side_busy ? s_grid_side : s_grid);
    {
        TimedLaunch tl(c, T_DIFF, s3);
        /* a proposal that leaves slope and amplitude alone (d_max, trans level): the kernel without transcendental functions; the
         * device has the last word (DiffConst.zdy: the other kernel's pass comes out void) */
        const bool zdy = hp.slope == c->par_model.slope && hp.c1 == c->par_model.c1 && hp.fact == c->par_model.fact;
        ++c->diff_seq;
        if (zdy)
            hipLaunchKernelGGL(k_full_diff_tiled<true>, dim3(grid), dim3(DIFF_THREADS), sizeof(DiffLds), s3, c->tile_work, c->tiled_cc, c->tabrec,
                               c->diff_const, c->M, c->scratch_diff, c->n_tile_static, (TileDyn*)c->tile_dyn, c->tile_dyn_list, c->host_nuis_dev,
                               c->diff_seq, c->tile_partial, c->tile_partial0, n_trans, c->scratch_nuis, c->diff_trace);
        else
            hipLaunchKernelGGL(k_full_diff_tiled<false>, dim3(grid), dim3(DIFF_THREADS), sizeof(DiffLds), s3, c->tile_work, c->tiled_cc, c->tabrec,
                               c->diff_const, c->M, c->scratch_diff, c->n_tile_static, (TileDyn*)c->tile_dyn, c->tile_dyn_list, c->host_nuis_dev,
                               c->diff_seq, c->tile_partial, c->tile_partial0, n_trans, c->scratch_nuis, c->diff_trace);
    }
    c->nuis_tier = 1;
    if (g_nuis_screen_verify) { /* the exact pass behind it, unconditionally */
        launch_nuis_exact_tiles(c, s3);
        c->nuis_exact_queued = true;
    }
    return 0;
}

/* tier 0: the histogram (built here if it is not valid: the first step of a run, or after moves outside one), its evaluation and
 * the zero-pixel sum of the test set in one launch */
static int launch_nuis_hist(ig_ctx* c, hipStream_t s3)
{
    if (ensure_nuis_hist(c)) return -1;
    if (!c->nh_valid) {
        HIPCK(hipMemsetAsync(c->nh.bins, 0, (size_t)NH_NB * 4 * sizeof(long long), s3));
        HIPCK(hipMemsetAsync(c->nh.dh, 0, ((size_t)c->nh.dh_n + 1) * sizeof(long long), s3));
        HIPCK(hipMemsetAsync(c->nh.misc, 0, NH_MISC * sizeof(long long), s3));
        hipLaunchKernelGGL(k_hist_build, dim3(2048), dim3(256), 0, s3, c->rowptr, c->cc, c->tab_prev, c->M, c->nh);
        c->nh_valid = true;
        c->nhs[7] += 1.0;
    }
    const int n_zero = std::min(256, std::max(32, c->M / 1024));
    ++c->diff_seq;
    hipLaunchKernelGGL(k_hist_eval, dim3(n_zero + NH_NB / 256 + NH_DH_BLOCKS), dim3(256), 0, s3, c->nh, c->glob, c->full_const, c->score_const,
                       c->diff_const, c->scratch_hist, c->host_nuis_dev, c->diff_seq, c->tab_prev, c->M, c->scratch_nuis + 2, n_zero, c->scratch_nuis,
                       PzTab{c->pz_tab1, c->pz_n1}, PzTab{c->pz_tab, c->pz_n});
    c->nuis_tier = 0;
    return 0;
}

/* a step's screened pass: the tier it starts with */
static int launch_nuis_screened(ig_ctx* c, const ig_params& hp, float mean_kb, hipStream_t s3, bool fuse_catch)
{
    if (launch_nuis_prepare(c, hp, mean_kb, s3, fuse_catch)) return -1;
    c->nuis_diff = true;
    c->nuis_exact_queued = false;
    c->nuis_pub_sums = false;
    if (nuis_hist_usable(c)) return launch_nuis_hist(c, s3);
    return launch_nuis_diff(c, hp, s3, true);
}

/* tab_prev := the state before the move about to be decided, then (second stream) the full pass under p_test on it */
static int enqueue_nuis_pass(ig_ctx* c, const float p_test[8], float mean_subfrag_kb)
{
    if (ensure_host_nuis(c)) return -1;
    if (!c->pz_tab1) DALLOC(c->pz_tab1, PZ_MAX);
    if (nh_flush_pending(c)) return -1; /* (before tab_prev catches up with the last move) */
    /* the nuisance pass first (second stream), the move behind it (library stream): the pass is the longer of the two and
     * would otherwise start only when the host is through with the move's dozen launches */
    hipStream_t s3 = c->stream3;
    bool on_side = false, fuse_catch = false;
    const bool use_diff = nuis_screen_usable(c);
    if (!c->nuis_caught_up) {
        if (c->main_drained && use_diff) {
            fuse_catch = on_side = true; /* the screened pass's first launch does it (k_nuis_prepare), see launch_nuis_diff */
        } else if (c->main_drained) {
            /* nothing is queued on the library stream (the previous step's results are on the host, nothing was promoted since):
             * the catch-up runs at the head of the pass's own stream -- an event from the library stream to this one costs ~15 us
             * of idle queue at the start of every step -- and the library stream's next kernels, which replace what it reads,
             * wait for IT (that wait is not on the step's critical path) */
            hipLaunchKernelGGL(k_catch_up, dim3(16), dim3(256), 0, s3, c->tab, c->tab_prev, c->prev_touched, c->glob);
            HIPCK(hipEventRecord(c->ev_main, s3));
            HIPCK(hipStreamWaitEvent(c->stream, c->ev_main, 0));
            on_side = true;
        } else {
            hipLaunchKernelGGL(k_catch_up, dim3(16), dim3(256), 0, c->stream, c->tab, c->tab_prev, c->prev_touched, c->glob);
            HIPCK(hipEventRecord(c->ev_gathered, c->stream)); /* also: behind an accepted step's kernels (ig_nuis_accept), which read what the pass overwrites */
        }
    }
    c->nuis_caught_up = false;
    c->main_drained = false;
    const ig_params hp = {p_test[0], p_test[1], p_test[2], p_test[3], p_test[4], p_test[5], p_test[6], p_test[7]};
    c->nuis_test = hp;
    c->nuis_mean_kb = mean_subfrag_kb;
    const double need = (mean_subfrag_kb > 0) ? (double)p_test[5] / (double)mean_subfrag_kb + 2.0 : 0.0;
    c->pz_n1 = (need > 0 && need < (double)PZ_MAX) ? (int)need : ((need >= (double)PZ_MAX) ? PZ_MAX : 0);
    if (!on_side) HIPCK(hipStreamWaitEvent(s3, c->ev_gathered, 0));
    c->nuis_pub_sums = false;
    c->nuis_diff = false;
    c->nuis_screen_rejected = false;
    if (use_diff) return launch_nuis_screened(c, hp, mean_subfrag_kb, s3, fuse_catch);
    c->pub_sums = (c->nuis_spec && c->host_nuis_dev) ? c->host_nuis_dev : nullptr; /* launch_full_nz: the tiled kernel's last workgroup publishes */
    const bool zero_done = launch_full_nz(c, c->tab_prev, 1, c->scratch_nuis, PzTab{c->pz_tab1, c->pz_n1}, s3, c->scratch_nuis + 2, &hp, mean_subfrag_kb);
    c->pub_sums = nullptr;
    if (!zero_done) hipLaunchKernelGGL(k_full_zero, dim3(128), dim3(256), 0, s3, c->tab_prev, c->glob, 1, c->M, c->scratch_nuis + 2);
    if (!c->nuis_pub_sums) HIPCK(hipMemcpyAsync(c->host_nuis->sums, c->scratch_nuis, 8 * sizeof(long long), hipMemcpyDeviceToHost, s3));
    return 0;
}

extern "C" int ig_nuis_begin(ig_ctx* c, int32_t frag_a, const int32_t* cands, int32_t C, const float p_test[8], float mean_subfrag_kb)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (c->world > 1) return fail("ig_nuis_begin: this handle scores a contact shard");
    if (c->nuis_in_flight) return fail("ig_nuis_begin: the previous step was not ended (ig_nuis_end)");
    nuis_latch_env();
    if (validate_move(c, frag_a, cands, C)) return -1;
    if (ensure_move_buffers(c, std::max(8, (int)C))) return -1;
    if (ensure_io(c, 1, C)) return -1;
    if (ensure_host_nuis(c)) return -1;
    c->host_nuis->frag = frag_a;
    for (int i = 0; i < C; i++) c->host_nuis->cands[i] = cands[i];
    if (upload_one_move(c, &c->host_nuis->frag, c->host_nuis->cands, C)) return -1;
    c->nuis_in_flight = true;
    c->nuis_spec = false;
    c->spec_valid = false;
    c->spec_slot = 0;
    c->nuis_one_C = C;
    if (enqueue_nuis_pass(c, p_test, mean_subfrag_kb)) return -1;
    /* the move */
    if (enqueue_move(c, 0, C, -1, 2)) return -1;
    enqueue_apply(c, 0, 0, 0);
    HIPCK(hipMemcpyAsync(&c->host_nuis->res, c->d_results, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
    if (queue_max_readback(c)) return -1;
    HIPCK(hipGetLastError());
    return 0;
}

/* ---- the same for a RUN of (move, nuisance step) pairs, the moves scored ahead in speculative batches ----------------------
 * A rejected nuisance step changes nothing a move reads, so the moves behind it can be scored before its outcome is
 * known: ig_nuis_run_begin uploads the lists of the run; ig_nuis_step_begin(i) enqueues step i's pass, scores a batch of
 * moves starting at i if move i has no valid scores yet (first step, after an accepted step, after a conflict, batch used
 * up), and decides + applies move i ALONE from its records (k_decide_batch over one slot); ig_nuis_end / ig_nuis_accept as
 * above.  An accepted step invalidates the slots scored ahead.  Same results as one move and one step at a time. */
static int nuis_spec_width(ig_ctx* c, int slots)
{
    if (g_nuis_w < 0) g_nuis_w = 0; /* (IG_NUIS_W: nuis_latch_env) */
    const int s_w = g_nuis_w;
    const int cap = std::min(slots, IG_MAX_BATCH);
    if (s_w > 0) return std::min(s_w, cap);
    if (c->spec_ema <= 0.0) c->spec_ema = 3.0;
    return std::max(1, std::min(cap, (int)(1.5 * c->spec_ema + 1.5)));
}

/* 1: the initial prev / next arrays (ig_upload_state / ig_set_initial_genome) are mutually inverse -- what the batch commit's
 * genome-distance bookkeeping relies on; 0: moves are applied one at a time */
extern "C" int ig_links_inverse(ig_ctx* c) { IG_JOIN(c); return c->init_links_inverse ? 1 : 0; }

extern "C" int ig_set_nuis_width(int w)
{
    g_nuis_w = std::max(0, w);
    return 0;
}

extern "C" int ig_nuis_run_begin(ig_ctx* c, int32_t n_moves, const int32_t* frags, const int32_t* cands, int32_t max_c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (c->world > 1) return fail("ig_nuis_run_begin: this handle scores a contact shard");
    if (c->nuis_in_flight) return fail("ig_nuis_run_begin: a step is in flight (ig_nuis_end)");
    nuis_latch_env();
    if (n_moves <= 0) return fail("ig_nuis_run_begin: no moves");
    if (max_c < 1 || max_c > IG_MAX_CANDIDATES) return fail("ig_nuis_run_begin: max_c out of range");
    if (!c->init_links_inverse) return fail("ig_nuis_run_begin: the initial prev / next arrays are not mutually inverse (ig_links_inverse): ig_nuis_begin, one pair at a time");
    if (nh_flush_pending(c)) return -1; /* the last move of the run before: into the histogram while its slot is still there */
#ifndef NUIS_S_CAP
#define NUIS_S_CAP 24
#endif
    const int s_cap = NUIS_S_CAP; /* (wider structural batches: 40 / 64 slots 8.7 / 8.0 k instead of 9.1 k in round 3; with chains 32 / 40 / 48 slots: 16.7 / 17.1 / 16.7 k against 17.3 k) */
    if (g_nuis_w < 0) g_nuis_w = 0; /* (IG_NUIS_W: nuis_latch_env) */
    const int Wmax = std::max(1, std::min(std::max(s_cap, g_nuis_w), max_batch_width(c, max_c)));
    if (ensure_move_buffers(c, std::max(8, (int)max_c), Wmax)) return -1;
    if (upload_moves(c, n_moves, frags, cands, max_c)) return -1;
    c->nuis_spec = true;
    c->spec_valid = false;
    c->spec_prev_pending = false;
    c->spec_base = c->spec_W = c->spec_next = c->spec_move = c->spec_slot = 0;
    c->spec_par_begin = c->spec_par_end = 0;
    c->full_windows = false;
    return 0;
}

/* Widths.  The PARAMETER width (slots screened / scored per launch) follows the number of moves decided between two accepted
 * steps; the STRUCTURAL width (slots gathered, mutated and sliced per launch) the number of moves a batch gets through before
 * a conflict -- an accepted step voids only the former.  IG_NUIS_W / ig_set_nuis_width fixes both (tests).  `slots`: what the window
 * buffers hold, from the call that ensured them (nuis_spec_score) */
static int nuis_struct_width(ig_ctx* c, int slots)
{
    const int cap = std::min(slots, IG_MAX_BATCH);
    if (g_nuis_w > 0) return std::min(g_nuis_w, cap);
    if (c->spec_struct_ema <= 0.0) c->spec_struct_ema = cap;
    /* (not "at least the parameter width": that one follows the runs between accepted steps now, and where a batch ends in a conflict
     * after two moves -- few long contigs -- slots gathered, mutated and sliced behind it are wasted) */
    return std::min(cap, std::max(2, (int)(1.5 * c->spec_struct_ema + 1.5))); /* (at least two where two fit) */
}

/* the parameter-dependent scores ahead are of no use any more (accepted step) */
static void nuis_par_invalidate(ig_ctx* c)
{
    c->spec_par_begin = c->spec_par_end = c->spec_next;
}
/* spec_ema: the moves decided between two accepted steps, moving average (what a piece scored under one parameter set is good
 * for).  Until round 4 it was fed with the use a PIECE got, which a conflict or the end of a batch cuts short as well: a settled
 * chain (one accepted step in 30) scored its parameter halves in pieces of 6 slots, 650 re-scorings for 3 600 steps. */
static void nuis_run_length(ig_ctx* c, bool accepted)
{
    if (accepted) {
        c->spec_ema = 0.7 * (c->spec_ema > 0 ? c->spec_ema : 3.0) + 0.3 * (double)c->since_accept;
        c->since_accept = 0;
    } else if ((double)c->since_accept > c->spec_ema) { /* (a run longer than the average already: no need to wait for its end) */
        c->spec_ema = 0.9 * c->spec_ema + 0.1 * (double)c->since_accept;
    }
}

/* the batch in the buffers is of no use any more (conflict, used up, a run's end) */
static void nuis_spec_invalidate(ig_ctx* c)
{
    if (c->spec_valid && c->spec_W > 0) {
        const double len = (c->spec_next >= c->spec_W) ? 2.0 * c->spec_W : (double)c->spec_next;
        c->spec_struct_ema = 0.7 * (c->spec_struct_ema > 0 ? c->spec_struct_ema : (double)c->spec_W) + 0.3 * len;
        nuis_par_invalidate(c);
    }
    c->spec_valid = false;
}

/* score a batch of moves starting at `move`: the structural half of all its slots, the parameter half of the first ones */
/* chains of pairs decided on the device (ig_nuis_chain_begin): 1 (default; env IG_NUIS_CHAIN, ig_set_nuis_chain): the runs predict
 * the windowed winners' deltas while they score (a pending move would end a chain) */
static bool nuis_chain_on() { return g_nuis_chain != 0; }
extern "C" int ig_set_nuis_chain(int on)
{
    g_nuis_chain = on ? 1 : 0;
    return 0;
}

static int nuis_spec_score(ig_ctx* c, int move)
{
    if (nh_flush_pending(c)) return -1; /* (the buffers of the last move's slot are about to be overwritten) */
    nuis_spec_invalidate(c);
    const int held = ensure_window_slots(c); /* the longest contig may have grown: the buffers first, the widths from what they hold */
    if (held < 0) return -1;
    const int W = std::min(nuis_struct_width(c, held), c->up_moves - move);
    const int r = std::min(nuis_spec_width(c, held), W);
    c->no_predict = !(nuis_chain_on() && nuis_hist_usable(c)); /* (decided one move per step: a pause for a windowed winner costs nothing the step would not wait for anyway; a chain would end at it) */
    const int rc = enqueue_score(c, move, W, c->up_max_c, -1, 2, 0, W, 0, r, false);
    c->no_predict = false;
    if (rc) return -1;
    c->spec_base = move;
    c->spec_W = W;
    c->spec_next = 0;
    c->spec_par_begin = 0;
    c->spec_par_end = r;
    c->spec_valid = true;
    c->spec_prev_pending = false;
    return 0;
}

/* the structural half of the batch stands (no conflict so far, slots left): the parameter half of the next slots -- after an
 * accepted step (new parameters), or because the piece scored before is used up */
static bool nuis_spec_can_rescore(const ig_ctx* c, int move)
{
    return c->spec_valid && c->spec_next < c->spec_W && c->spec_base + c->spec_next == move;
}
static int nuis_spec_rescore(ig_ctx* c)
{
    nuis_par_invalidate(c);
    /* (NOT ensure_window_slots: the structural half of the batch lives in the buffers as they are -- what they hold is the cap) */
    const int pb = c->spec_next, pe = std::min(c->spec_W, pb + nuis_spec_width(c, slots_held(c)));
    c->no_predict = !(nuis_chain_on() && nuis_hist_usable(c));
    const int rc = enqueue_score(c, c->spec_base, c->spec_W, c->up_max_c, -1, 2, 0, c->spec_W, pb, pe, true);
    c->no_predict = false;
    if (rc) return -1;
    c->spec_par_begin = pb;
    c->spec_par_end = pe;
    return 0;
}

extern "C" int ig_nuis_step_begin(ig_ctx* c, int32_t move, const float p_test[8], float mean_subfrag_kb)
{
    IG_JOIN(c);
    return nuis_step_begin_impl(c, move, p_test, mean_subfrag_kb);
}
static int nuis_step_begin_impl(ig_ctx* c, int32_t move, const float p_test[8], float mean_subfrag_kb)
{
    HIPCK(hipSetDevice(c->device));
    if (!c->nuis_spec) return fail("ig_nuis_step_begin: no run (ig_nuis_run_begin)");
    if (c->nuis_in_flight) return fail("ig_nuis_step_begin: the previous step was not ended (ig_nuis_end)");
    if (move != c->spec_move || move >= c->up_moves) return fail("ig_nuis_step_begin: move %d, expected %d of %d", move, c->spec_move, c->up_moves);
    c->nuis_in_flight = true;
    c->nh_tracking = true; /* until the step is ended: the one move it applies is walked into the histogram at the head of the next step */
    /* a batch is scored in this step (or still being scored: right after an accepted step): the pass leaves half of every CU
     * to it; else it takes the machine (all that runs next to it is one decision and one apply) */
    const bool restruct = !nuis_spec_can_rescore(c, move);
    const bool repar = !restruct && c->spec_next >= c->spec_par_end; /* the piece scored under the current parameters is used up */
    c->side_busy = restruct || repar || c->spec_next == c->spec_par_begin;
    if (enqueue_nuis_pass(c, p_test, mean_subfrag_kb)) return -1;
    c->side_busy = true;
    if (restruct) {
        if (nuis_spec_score(c, move)) return -1;
    } else if (repar) {
        if (nuis_spec_rescore(c)) return -1;
    }
    /* the result record reaches the host as soon as the move is applied: written by k_commit_batch itself where the host
     * memory is mapped, else copied (and copied in the rare cases ig_nuis_end has to redo the move) */
    c->nuis_pub_res = c->host_nuis_dev != nullptr;
    launch_commit(c, c->spec_base, c->spec_next + 1, c->spec_next, c->spec_prev_pending ? 0 : 1, c->nuis_pub_res);
    if (!c->nuis_pub_res) {
        HIPCK(hipMemcpyAsync(&c->host_nuis->res, c->d_results + move, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
        if (queue_max_readback(c)) return -1;
    }
    HIPCK(hipGetLastError());
    return 0;
}

/* the host half of a step of a run: the decision of move spec_move is in (or the slot has to be scored again) */
static int nuis_spec_finish(ig_ctx* c)
{
    bool redone = false;
    for (int attempt = 0;; attempt++) {
        int bo[16];
        const int w = c->spec_next;
        if (wait_commit(c, bo, w == c->spec_par_begin, w)) return -1;
        if (c->own_screened == 1 && w == c->spec_par_begin && !(bo[2] && bo[0] == 0 && bo[1] < 0)) size_exact_grid(c, bo);
        if (bo[0] == w + 1) {
            c->spec_prev_pending = false;
            break;
        }
        if (bo[1] == w) { /* a windowed winner without a predicted delta: the one-move tail */
            enqueue_apply(c, c->spec_base + w, w, 0, true); /* (its contigs onto the batch's list of modified ones) */
            c->n_batch_pending++;
            c->spec_prev_pending = false;
            redone = true;
            break;
        }
        /* not decided: a contig of the move was modified by an earlier move of the batch (w > 0), or the first slot did not
         * fit the slice pool / the exact kernel's grid: score a batch from this move */
        if (w == 0) {
            if (bo[2] < 1 || bo[2] > 3) {
                Glob hg;
                HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
                return fail("device-side consistency failure %d at move %d of a run", hg.error, c->spec_move);
            }
            if (make_room(c, bo[2], "the first move of a batch")) return -1;
            c->spec_valid = false; /* says nothing about run lengths */
        }
        if (attempt > 8) return fail("move %d of a run could not be decided", c->spec_move);
        if (nuis_spec_score(c, c->spec_move)) return -1;
        launch_commit(c, c->spec_base, 1, 0, 0);
        redone = true;
    }
    c->spec_slot = c->spec_next;
    c->nuis_nzb_copied = false;
    if (redone) {
        c->nuis_pub_res = false;
        HIPCK(hipMemcpyAsync(&c->host_nuis->res, c->d_results + c->spec_move, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
        /* ... and the maintained sum of the state the move was decided against (the decide step left it in the slot's control
         * block): the step's screened pass starts from it */
        HIPCK(hipMemcpyAsync((void*)c->host_nuis->nzb, &c->mb.ctl[c->spec_slot].nzb_hi, 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        c->nuis_nzb_copied = true;
        if (queue_max_readback(c)) return -1;
    }
    c->spec_next++;
    c->spec_move++;
    c->since_accept++;
    nuis_run_length(c, false);
    return 0;
}

/* z of a pass from its eight sums (as ig_full_likelihood) */
static double nuis_z_from_sums(const long long h_in[8])
{
    long long h[8];
    memcpy(h, h_in, sizeof h);
    ig_acc_normalize((int64_t*)&h[2], (int64_t*)&h[3]);
    const double log_e = 0.43429448190325182;
    double n_tot_pxl;
    float v_inter;
    const int vi_bits = (int)h[7];
    memcpy(&n_tot_pxl, &h[5], sizeof n_tot_pxl);
    memcpy(&v_inter, &vi_bits, sizeof v_inter);
    return ig_acc_to_double(h[2], h[3]) * log_e + log_e * (n_tot_pxl - (double)h[4]) * -1.0 * (double)v_inter;
}

/* Tu = {temperature, u} of the Metropolis test when the caller is ig_nuis_step_next: a step whose screened interval lies
 * below T ln u is rejected without the exact pass (nuis_screen_rejected; *nz_test is then the interval's midpoint) */
static int nuis_end_body(ig_ctx* c, ig_move_result* out, double* nz_test, double* z_test, int64_t* limbs5, const double* Tu);
static int nuis_end_impl(ig_ctx* c, ig_move_result* out, double* nz_test, double* z_test, int64_t* limbs5, const double* Tu)
{
    const int rc = nuis_end_body(c, out, nz_test, z_test, limbs5, Tu);
    c->nh_tracking = false;
    if (rc) { /* (whatever went wrong: the histogram is rebuilt by the next step that wants it) */
        c->nh_valid = false;
        c->nh_pending_slot = -1;
    }
    return rc;
}
static int nuis_end_body(ig_ctx* c, ig_move_result* out, double* nz_test, double* z_test, int64_t* limbs5, const double* Tu)
{
    HIPCK(hipSetDevice(c->device));
    if (!c->nuis_in_flight) return fail("ig_nuis_end: no step in flight");
    c->nuis_in_flight = false;
    c->nuis_screen_rejected = false;
    c->nuis_accept_certain = false;
    const auto w0 = std::chrono::steady_clock::now();
    if (c->nuis_spec && nuis_spec_finish(c)) return -1;
    bool have_nzb = false;
    int moved = 1; /* the move changed the genome (0 only when k_commit_batch said so) */
    c->last_moved = true;
    if (c->nuis_spec && c->nuis_pub_res && wait_host_flag(&c->host_nuis->res_seq, c->res_seq, c->stream)) {
        c->max_L = std::max(c->max_L, c->host_nuis->max_L);
        c->max_SL = std::max(c->max_SL, c->host_nuis->max_SL);
        have_nzb = true; /* the record came from k_commit_batch, with the maintained sum of the state before the move */
        moved = c->host_nuis->changed;
        c->last_moved = moved != 0;
    } else {
        if (c->nuis_spec && c->nuis_pub_res) { /* no flag although the stream has drained: fetch the record the plain way */
            HIPCK(hipMemcpyAsync(&c->host_nuis->res, c->d_results + c->spec_move - 1, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
            if (queue_max_readback(c)) return -1;
        }
        HIPCK(hipStreamSynchronize(c->stream));
        take_max_readback(c);
        while (!c->nuis_spec && c->host_nuis->res.pad == 1) { /* ig_nuis_begin's move through the one-move kernels: its lists did not fit the
                                                                * slice pool and nothing was applied -- the move again with a larger pool (the
                                                                * step's pass read the state before the move: it stands) */
            if (retry_with_larger_pool(c)) return -1;
            if (enqueue_move(c, 0, c->nuis_one_C, -1, 2)) return -1;
            enqueue_apply(c, 0, 0, 0);
            HIPCK(hipMemcpyAsync(&c->host_nuis->res, c->d_results, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
            if (queue_max_readback(c)) return -1;
            HIPCK(hipStreamSynchronize(c->stream));
            take_max_readback(c);
        }
        have_nzb = c->nuis_spec && c->nuis_nzb_copied;
    }
    /* the screened pass: decide from its interval where that is possible -- the histogram's first (tier 0), then the float pass
     * over the contacts (tier 1), then the exact pass */
    bool scr_valid = false, scr0_valid = false;
    double scr_mid = 0.0, scr_B = 0.0, scr0_mid = 0.0, scr0_B = 0.0;
    if (c->nuis_diff) {
        NuisHost* hn = c->host_nuis;
        bool reject = false, accept = false;
        c->nscr[0] += 1.0;
        for (;;) {
            const int tier = c->nuis_tier;
            if (!wait_host_flag(&hn->diff_seq, c->diff_seq, c->stream3)) {
                HIPCK(hipStreamSynchronize(c->stream3));
                if (tier == 0) { /* (its words are cleared by the launch itself: the copies it leaves) */
                    long long t3[3];
                    HIPCK(hipMemcpy(t3, c->scratch_hist + 9, sizeof t3, hipMemcpyDeviceToHost));
                    for (int q = 0; q < 8; q++) hn->diff[q] = 0;
                    hn->diff[2] = t3[0];
                    hn->diff[3] = t3[1];
                    hn->diff[4] = t3[2];
                } else {
                    HIPCK(hipMemcpy((void*)hn->diff, c->scratch_diff, 8 * sizeof(long long), hipMemcpyDeviceToHost));
                }
                HIPCK(hipMemcpy((void*)hn->sums, c->scratch_nuis, 8 * sizeof(long long), hipMemcpyDeviceToHost));
            }
            long long d[8];
            memcpy(d, (const void*)hn->diff, sizeof d);
            scr_valid = false;
            if (tier == 0) c->nhs[0] += 1.0;
            if (d[4] != 0 || d[3] <= 0 || !have_nzb) {
                if (tier == 0) {
                    c->nhs[3] += 1.0;
                    if (g_nuis_hist_trace)
                        fprintf(stderr, "[nuis] move %d: histogram tier void: flags %lld sum %lld bound %lld contacts %lld record %d\n", c->spec_move - 1,
                                d[4], d[2], d[3], d[5], (int)have_nzb);
                    if (d[4] & 1) c->nhs[8] += 1.0;
                    if (d[4] & 2) c->nhs[9] += 1.0;
                    if (d[4] & 4) c->nhs[10] += 1.0;
                    if (!have_nzb) c->nhs[11] += 1.0;
                } else {
                    c->nscr[3] += 1.0; /* void: outside the screening term's domain, or the move did not come out of the batch commit */
                    if (d[4] & 1) c->nscr[8] += 1.0;  /* ... the parameter pair (one-log domain, size of the proposal) */
                    if (d[4] & 2) c->nscr[9] += 1.0;  /* ... a contact (ring, count, rank distance beyond the tables) */
                    if (d[4] & 4) c->nscr[10] += 1.0; /* ... a workgroup's sums (|log2 s|, |y|, not a number) */
                    if (!have_nzb) c->nscr[11] += 1.0;
                }
            } else {
                long long hi = hn->nzb[0] + d[0], lo = hn->nzb[1] + d[1];
                ig_acc_normalize((int64_t*)&hi, (int64_t*)&lo);
                const double base = ig_acc_to_double(hi, lo);
                scr_mid = base + (double)d[2] * (1.0 / DIFF_FIX);
                scr_B = (double)d[3] * (1.0 / DIFF_FIX) + 1e-6 + 1e-14 * (__builtin_fabs(base) + __builtin_fabs(hn->res.o)); /* + the double roundings here */
                scr_valid = true;
                if (tier == 0) {
                    c->nhs[4] += scr_B;
                } else {
                    c->nscr[4] = std::max(c->nscr[4], scr_B);
                    c->nscr[6] += scr_B;
                }
                if (Tu && Tu[0] > 0.0 && Tu[1] > 0.0 && !g_nuis_screen_verify) {
                    const double z = nuis_z_from_sums((const long long*)hn->sums);
                    const double x_hi = (((scr_mid + scr_B) + z) - hn->res.o) / Tu[0], x_lo = (((scr_mid - scr_B) + z) - hn->res.o) / Tu[0];
                    reject = exp(x_hi) <= Tu[1] * (1.0 - 1e-9); /* exp is monotone: every L_test in the interval gives a ratio below u */
                    accept = !reject && exp(x_lo) >= Tu[1] * (1.0 + 1e-9) && c->host_nuis_dev; /* ... above it: accepted whatever the exact sum */
                }
            }
            if (tier == 0) {
                if (reject) c->nhs[1] += 1.0;
                if (accept) c->nhs[2] += 1.0;
                if (!reject && !accept) { /* the histogram does not decide (or the check wants every tier): the pass over the contacts */
                    scr0_valid = scr_valid;
                    scr0_mid = scr_mid;
                    scr0_B = scr_B;
                    if (launch_nuis_diff(c, c->nuis_test, c->stream3, false)) return -1;
                    continue;
                }
            }
            break;
        }
        if (scr_valid && !reject && !accept) c->nscr[7] += 1.0;
        if (accept) {
            /* the exact pass is needed -- for the maintained sum under the new parameters and for the likelihood the step
             * returns -- but not for the decision: it runs on the side stream while the library stream promotes the parameters
             * and re-scores the moves ahead; its sums are promoted in front of the next kernel that reads the maintained sum
             * (flush_pending_sums), the caller fetches the exact value later (ig_nuis_exact_result) */
            if (!c->scratch_exact) {
                DALLOC(c->scratch_exact, 8);
                HIPCK(memset_now(c->scratch_exact, 0, 8 * sizeof(long long)));
            }
            c->nscr[2] += 1.0;
            if (!c->nuis_tiles_listed) launch_nuis_tile_list(c, c->stream3, false);
            launch_nuis_exact_tiles(c, c->stream3, c->scratch_exact, false);
            HIPCK(hipEventRecord(c->ev_exact, c->stream3));
            c->nuis_sums_pending = true;
            c->nuis_accept_certain = true;
        }
        if (reject) {
            c->nscr[1] += 1.0;
            c->nuis_screen_rejected = true;
        }
        if (reject || accept) {
            c->nuis_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
            HIPCK(hipGetLastError());
            drain_timers(c);
            c->main_drained = c->nuis_spec;
            *out = hn->res;
            if (out->error) return fail("device-side consistency failure %d", out->error);
            if (c->nuis_spec) c->nh_pending_slot = (c->nh_valid && moved) ? c->spec_slot : -1;
            if (c->nuis_spec) c->nh_p_changed = 0.98 * c->nh_p_changed + 0.02 * (moved ? 1.0 : 0.0);
            if (nz_test) *nz_test = scr_mid;
            if (z_test) *z_test = nuis_z_from_sums((const long long*)hn->sums);
            if (limbs5)
                for (int i = 0; i < 5; i++) limbs5[i] = 0;
            return 0;
        }
        c->nscr[2] += 1.0;
        if (!c->nuis_exact_queued) { /* the exact pass over the same list of tiles */
            if (!c->nuis_tiles_listed) launch_nuis_tile_list(c, c->stream3, false);
            launch_nuis_exact_tiles(c, c->stream3);
        }
    }
    if (!(c->nuis_spec && c->nuis_pub_sums && wait_host_flag(&c->host_nuis->sums_seq, c->sums_seq, c->stream3))) {
        if (c->nuis_spec && c->nuis_pub_sums)
            HIPCK(hipMemcpyAsync(c->host_nuis->sums, c->scratch_nuis, 8 * sizeof(long long), hipMemcpyDeviceToHost, c->stream3));
        HIPCK(hipStreamSynchronize(c->stream3));
    }
    c->nuis_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count(); /* ig_debug_nuis_wait */
    HIPCK(hipGetLastError());
    drain_timers(c);
    c->main_drained = c->nuis_spec; /* a run's step: its last kernel on the library stream has delivered (or the stream was synchronised) */
    *out = c->host_nuis->res;
    if (out->error) return fail("device-side consistency failure %d", out->error);
    if (c->nuis_spec) c->nh_pending_slot = (c->nh_valid && moved) ? c->spec_slot : -1; /* (the histogram follows the move at the head of the next step) */
    if (c->nuis_spec) c->nh_p_changed = 0.98 * c->nh_p_changed + 0.02 * (moved ? 1.0 : 0.0); /* (the histogram tier's cost model, nuis_hist_usable) */
    if (scr_valid || scr0_valid) { /* the exact pass ran as well: how much of the bounds did the screened sums use?  (verify mode: the check) */
        long long e[2] = {c->host_nuis->sums[0], c->host_nuis->sums[1]};
        ig_acc_normalize((int64_t*)&e[0], (int64_t*)&e[1]);
        const double exact = ig_acc_to_double(e[0], e[1]);
        static const int s_nocheck = getenv("IG_NUIS_SCREEN_NOCHECK") ? atoi(getenv("IG_NUIS_SCREEN_NOCHECK")) : 0; /* tuning builds that compute garbage */
        if (scr_valid) {
            const double err = __builtin_fabs(scr_mid - exact);
            if (scr_B > 0.0) c->nscr[5] = std::max(c->nscr[5], err / scr_B);
            if (!(err <= scr_B) && !s_nocheck)
                return fail("screened nuisance pass: |screened - exact| = %.6g exceeds its bound %.6g (move %d)", err, scr_B, c->spec_move - 1);
        }
        if (g_nuis_hist_trace)
            fprintf(stderr, "[nuis] move %d exact %.9f  hist %s mid-exact %.3e B %.3e  pass %s mid-exact %.3e B %.3e\n", c->spec_move - 1, exact,
                    scr0_valid ? "ok" : "--", scr0_mid - exact, scr0_B, scr_valid ? "ok" : "--", scr_mid - exact, scr_B);
        if (scr0_valid) {
            const double err = __builtin_fabs(scr0_mid - exact);
            if (scr0_B > 0.0) c->nhs[5] = std::max(c->nhs[5], err / scr0_B);
            if (!(err <= scr0_B) && !s_nocheck)
                return fail("screened nuisance pass, histogram tier: |screened - exact| = %.6g exceeds its bound %.6g (move %d)", err, scr0_B, c->spec_move - 1);
        }
    }
    long long h[8];
    memcpy(h, (const void*)c->host_nuis->sums, sizeof h);
    ig_acc_normalize((int64_t*)&h[0], (int64_t*)&h[1]);
    ig_acc_normalize((int64_t*)&h[2], (int64_t*)&h[3]);
    if (nz_test) *nz_test = ig_acc_to_double(h[0], h[1]);
    if (z_test) { /* as ig_full_likelihood */
        const double log_e = 0.43429448190325182;
        double n_tot_pxl;
        float v_inter;
        const int vi_bits = (int)h[7];
        memcpy(&n_tot_pxl, &h[5], sizeof n_tot_pxl);
        memcpy(&v_inter, &vi_bits, sizeof v_inter);
        *z_test = ig_acc_to_double(h[2], h[3]) * log_e + log_e * (n_tot_pxl - (double)h[4]) * -1.0 * (double)v_inter;
    }
    if (limbs5)
        for (int i = 0; i < 5; i++) limbs5[i] = h[i];
    return 0;
}

extern "C" int ig_nuis_end(ig_ctx* c, ig_move_result* out, double* nz_test, double* z_test, int64_t* limbs5)
{
    IG_JOIN(c);
    return nuis_end_impl(c, out, nz_test, z_test, limbs5, nullptr);
}

/* {steps screened, rejected from the interval alone, exact passes behind a screened one, void, largest bound, largest used
 * fraction of a bound (where the exact pass ran), sum of the bounds, steps whose interval did not decide} since the handle was made */
extern "C" int ig_debug_nuis_screen_stats(ig_ctx* c, double out12[12])
{
    IG_JOIN(c);
    for (int i = 0; i < 12; i++) out12[i] = c->nscr[i];
    return 0;
}

/* the histogram tier: {evaluations, steps rejected there, accepted there, void, sum of its bounds, largest used fraction of a bound
 * (where the exact pass ran), moves walked into the histogram, builds from scratch} since the handle was made */
extern "C" int ig_debug_nuis_hist_stats(ig_ctx* c, double out12[12])
{
    IG_JOIN(c);
    for (int i = 0; i < 12; i++) out12[i] = c->nhs[i];
    return 0;
}

/* the maintained histogram against one built from scratch from the tables of the state it stands for (the state before the last
 * move of the run; the current state once that move has been walked in, which this call does): *mismatches = words that differ
 * (-1: no histogram) */
extern "C" int ig_debug_nuis_hist_check(ig_ctx* c, int64_t* mismatches)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    *mismatches = -1;
    if (c->nuis_in_flight) return fail("ig_debug_nuis_hist_check: a step is in flight");
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipStreamSynchronize(c->stream3));
    if (!c->nh.bins || !c->nh_valid) return 0;
    if (nh_flush_pending(c)) return -1;
    HIPCK(hipStreamSynchronize(c->stream3));
    const size_t nb = (size_t)NH_NB * 4, nd = (size_t)c->nh.dh_n + 1;
    NuisHist t{nullptr, nullptr, nullptr, c->nh.dh_n};
    DALLOC(t.bins, nb);
    DALLOC(t.dh, nd);
    DALLOC(t.misc, NH_MISC);
    HIPCK(memset_now(t.bins, 0, nb * sizeof(long long)));
    HIPCK(memset_now(t.dh, 0, nd * sizeof(long long)));
    HIPCK(memset_now(t.misc, 0, NH_MISC * sizeof(long long)));
    hipLaunchKernelGGL(k_hist_build, dim3(2048), dim3(256), 0, c->stream3, c->rowptr, c->cc, c->tab, c->M, t);
    HIPCK(hipStreamSynchronize(c->stream3));
    std::vector<long long> a(nb + nd + NH_MISC), b(nb + nd + NH_MISC);
    HIPCK(hipMemcpy(a.data(), c->nh.bins, nb * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(a.data() + nb, c->nh.dh, nd * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(a.data() + nb + nd, c->nh.misc, NH_MISC * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(b.data(), t.bins, nb * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(b.data() + nb, t.dh, nd * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(b.data() + nb + nd, t.misc, NH_MISC * sizeof(long long), hipMemcpyDeviceToHost));
    hipFree(t.bins);
    hipFree(t.dh);
    hipFree(t.misc);
    int64_t bad = 0;
    for (size_t i = 0; i < a.size(); i++)
        if (i != nb + nd + 7) bad += a[i] != b[i];
    bad += a[nb + nd + 7] < b[nb + nd + 7]; /* (the largest rank distance ever entered: a loop bound that never comes down) */
    *mismatches = bad;
    return 0;
}

/* the exact likelihood of the non-zero pixels under the test parameters of the last step that ig_nuis_step_next reported with
 * *accepted = 3 (decided from the screened interval, the exact pass behind the decision) */
extern "C" int ig_nuis_exact_result(ig_ctx* c, double* nz_test)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (c->exact_seq == 0 && !c->nuis_sums_pending) return fail("ig_nuis_exact_result: no step was accepted ahead of its exact pass");
    flush_pending_sums(c);
    NuisHost* hn = c->host_nuis;
    if (!hn) return fail("ig_nuis_exact_result: no run");
    if (!wait_host_flag(&hn->exact_seq, c->exact_seq, c->stream)) {
        HIPCK(hipStreamSynchronize(c->stream));
        if (hn->exact_seq != c->exact_seq) return fail("ig_nuis_exact_result: the promotion of the sums did not report");
    }
    *nz_test = ig_acc_to_double(hn->exact[0], hn->exact[1]);
    return 0;
}

/* the accepted step's parameters become the model's (CL:3032-3036) without another pass over all contacts: the maintained
 * exact sum under the new parameters on the CURRENT state = their full pass on the state before the last move (what the
 * step just evaluated, quirk Q12) + that move's exact delta under them (k_delta over the touched contigs); the zero-pixel sum
 * is recounted (O(M)) */
/* acc8: {zero-pixel hi, lo, pair count (k_full_zero), .., .., .., the move's delta hi, lo (k_delta)} -- all zero between two
 * accepted steps: the promotion clears what it has read.  One launch: thread 0 of block 0 promotes (parameters, maintained
 * sums), every block builds its share of the model's score / screening constants from the SAME parameters (set 1: what set 0
 * is being overwritten with), i.e. k_build_score_const and k_build_screen_const for the promoted set. */
/* mode 0: everything; 1: parameters, constants and the zero-pixel sum only (the exact pass over all contacts is still running:
 * ig_nuis_accept behind a decisively accepted step); 2: the maintained sum, once that pass is through (flush_pending_sums: one
 * block), its exact limbs to the host */
__global__ void __launch_bounds__(256) k_nuis_promote(Glob* g, long long* full_sums, long long* acc8, PzTab pz, const double* __restrict__ lgf_tab,
                                                      ScoreConst* score_const, ScreenConst* screen_const, int mode, NuisHost* hn, int hn_seq)
{
    if (mode != 2) {
        build_score_const_block(g, pz, lgf_tab, score_const, 1);
        build_screen_const_block(g, pz, screen_const, 1);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (mode != 2) {
            g->par[0] = g->par[1];
            long long h = acc8[0], l = acc8[1];
            ig_acc_normalize((int64_t*)&h, (int64_t*)&l);
            g->z_hi = h;
            g->z_lo = l;
            if (acc8[2] != g->n_intra) g->error = 8; /* the pair count does not depend on the parameters */
            for (int q = 0; q < 6; q++) acc8[q] = 0;
        }
        if (mode != 1) {
            long long h = full_sums[0] + acc8[6], l = full_sums[1] + acc8[7];
            ig_acc_normalize((int64_t*)&h, (int64_t*)&l);
            g->nz_hi = h;
            g->nz_lo = l;
            acc8[6] = acc8[7] = 0;
            if (mode == 2) {
                long long eh = full_sums[0], el = full_sums[1];
                ig_acc_normalize((int64_t*)&eh, (int64_t*)&el);
                for (int q = 0; q < 8; q++) full_sums[q] = 0; /* the side buffer of the deferred pass: zero between two uses */
                if (hn) {
                    hn->exact[0] = eh;
                    hn->exact[1] = el;
                    __threadfence_system();
                    hn->exact_seq = hn_seq;
                }
            }
        }
    }
}

/* the maintained sum of a decisively accepted step, as soon as something is about to read it: behind the exact pass (event) */
static void flush_pending_sums(ig_ctx* c)
{
    if (!c->nuis_sums_pending) return;
    c->nuis_sums_pending = false;
    hipStreamWaitEvent(c->stream, c->ev_exact, 0);
    hipLaunchKernelGGL(k_nuis_promote, dim3(1), dim3(64), 0, c->stream, c->glob, c->scratch_exact, c->scratch_accept, PzTab{c->pz_tab, c->pz_n}, c->lgf_tab,
                       c->score_const, c->screen_const, 2, c->host_nuis_dev, ++c->exact_seq);
}

extern "C" int ig_nuis_accept(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (c->nuis_in_flight) return fail("ig_nuis_accept: end the step first (ig_nuis_end)");
    if (!c->scratch_accept) {
        DALLOC(c->scratch_accept, 8);
        HIPCK(memset_now(c->scratch_accept, 0, 8 * sizeof(long long)));
    }
    long long* acc8 = c->scratch_accept;
    c->n_accepts++;
    c->main_drained = false;
    const int w = c->spec_slot; /* the slot of the move just applied (0 unless it came out of a batch: ig_nuis_step_begin) */
    /* whatever was scored ahead was scored under the old parameters -- but only its parameter-dependent half: windows, candidate
     * genomes, columns and slice lists of the batch's remaining slots stand (IG_NUIS_KEEP=0: redone as well) */
    nuis_run_length(c, true);
    if (c->nuis_spec) nuis_par_invalidate(c);
    else nuis_spec_invalidate(c);
    const PzTab pz1{c->pz_tab1, c->pz_n1};
    /* the move's delta under the new parameters; contig membership of the partners as of BEFORE the move: tab_prev.  A move that
     * left the genome as it was (91 % of them: k_commit_batch says so with the record) has none: 46 us of every accepted step */
    if (c->last_moved || !c->nuis_spec)
        hipLaunchKernelGGL(k_delta, dim3(DELTA_RB, 2, 1), dim3(SCORE_THREADS), 0, c->stream, c->rowptr, c->cc, c->tab_prev, c->tab_prev,
                           c->prev_touched, c->glob, c->mb, c->lgf_tab, pz1, w, 2, 1, acc8 + 6);
    hipLaunchKernelGGL(k_full_zero, dim3(128), dim3(256), 0, c->stream, c->tab, c->glob, 1, c->M, acc8, (const float*)c->pz_tab1, c->pz_n1);
    /* the promotion, and the tables of the model's parameter set: the test set's P_z table becomes the model's */
    c->par_model = c->nuis_test;
    std::swap(c->pz_tab, c->pz_tab1);
    std::swap(c->pz_n, c->pz_n1);
    const PzTab pz0{c->pz_tab, c->pz_n};
    hipLaunchKernelGGL(k_nuis_promote, dim3((LDS_PZ + 2 + 255) / 256), dim3(256), 0, c->stream, c->glob, c->scratch_nuis, acc8, pz0, c->lgf_tab,
                       c->score_const, c->screen_const, c->nuis_sums_pending ? 1 : 0, (NuisHost*)nullptr, 0);
    HIPCK(hipGetLastError());
    return 0;
}

/* ig_nuis_end, the Metropolis decision of step_nuisance_parameters (CL:3026-3036: ratio = exp((L_test - L_move) / T) >= u),
 * ig_nuis_accept and the next move's ig_nuis_step_begin in ONE call: between the end of a step's kernels and the first
 * launch of the next step there is no host code but this.  The caller supplies the next step's test parameters for both
 * outcomes (they are prepared while this step's kernels run; one of them may be NULL: then, on that outcome, the next step is
 * left to the caller's ig_nuis_step_begin -- the promotion's kernels run meanwhile).  *accepted: 0 / 1, or 2 when exp() lands within 1e-9
 * relative of u -- then nothing was decided or enqueued and the caller goes on with its own arithmetic (ig_nuis_accept,
 * ig_nuis_step_begin). */
extern "C" int ig_nuis_step_next(ig_ctx* c, double temperature, double u, const float p_next_rejected[8], const float p_next_accepted[8],
                                 float mean_subfrag_kb, int32_t has_next, ig_move_result* out, double* nz_test, double* z_test, int32_t* accepted)
{
    IG_JOIN(c);
    if (!c->nuis_spec) return fail("ig_nuis_step_next: no run (ig_nuis_run_begin)");
    double nz = 0.0, z = 0.0;
    const double Tu[2] = {temperature, u};
    if (nuis_end_impl(c, out, &nz, &z, nullptr, Tu)) return -1;
    if (nz_test) *nz_test = nz;
    if (z_test) *z_test = z;
    const double ratio = exp(((nz + z) - out->o) / temperature);
    int acc;
    if (c->nuis_screen_rejected) acc = 0; /* every L_test of the screened interval gives a ratio below u */
    else if (c->nuis_accept_certain) acc = 1; /* ... above u */
    else if (ratio != ratio) acc = 0; /* NaN >= u is false */
    else if (ratio >= u * (1.0 + 1e-9)) acc = 1;
    else if (ratio <= u * (1.0 - 1e-9)) acc = 0;
    else acc = 2;
    *accepted = (acc == 1 && c->nuis_accept_certain) ? 3 : acc; /* 3: accepted, *nz_test is the screened midpoint, the exact value through ig_nuis_exact_result */
    if (acc == 2) return 0;
    if (acc == 1 && ig_nuis_accept(c)) return -1;
    const float* p_next = acc ? p_next_accepted : p_next_rejected;
    if (has_next && p_next) return nuis_defer_step_begin(c, c->spec_move, p_next, mean_subfrag_kb); /* (on the helper thread: see NuisWorker) */
    /* the caller has yet to work out the next test parameters; what is certain is that the moves ahead have to be scored
     * under the parameters just promoted: that needs nothing from the caller, and runs while it computes */
    if (has_next && acc == 1 && c->spec_move < c->up_moves) {
        /* (first what the pass of the next step waits for, or it would queue behind the scoring launches) */
        if (nh_flush_pending(c)) return -1; /* (the histogram's walk of the last move reads tab_prev as of before it) */
        /* INVARIANT: behind a decisively accepted step the exact pass may still be running on the side stream (nuis_sums_pending) while
         * this catch-up rewrites tab_prev.len of the last move's contigs.  The pass reads tab_prev.len on its ring path only, and a ring
         * among the contacts voids both screened tiers (no decisive accept then: the exact pass ran in front of the decision).  Whoever
         * lets a ring through the screened tiers must order this launch behind ev_exact. */
        hipLaunchKernelGGL(k_catch_up, dim3(16), dim3(256), 0, c->stream, c->tab, c->tab_prev, c->prev_touched, c->glob);
        HIPCK(hipEventRecord(c->ev_gathered, c->stream)); /* (the next pass next to the scoring launches, not behind them: 4.8 k against 4.5 k) */
        c->nuis_caught_up = true;
        if (nuis_spec_can_rescore(c, c->spec_move)) {
            if (nuis_spec_rescore(c)) return -1;
        } else if (nuis_spec_score(c, c->spec_move)) {
            return -1;
        }
    }
    return 0;
}


/* ---- chains of (move, nuisance step) pairs decided on the device (ig_common.cuh: ChainIn; DESIGN.md 4.8) ------------------------
 * ig_nuis_chain_begin(move, n_sets, ...): the pairs move .. move + n_sets - 1 of the run, as far as the device can take them alone:
 * k_chain_prepare once (the sets' tables), then segment after segment (k_chain_hist_eval, k_chain_decide_commit on the library
 * stream; the histogram's walk of a move that changed the genome between two segments) until a pair needs the host.  Asynchronous (the
 * helper thread drives the segments; ig_nuis_chain_done polls, ig_nuis_chain_end waits): the caller prepares the proposals of the
 * steps behind meanwhile.  Every pair a chain completes is a move decided exactly as k_decide_batch decides it and a step
 * REJECTED from the histogram tier's interval with the margins of nuis_end_body; the pair a chain stops in front of is untouched. */
enum { CHAIN_R_SETS = 0, /* every set was used: the steps went through */
       CHAIN_R_TEST = 1,     /* the next pair's step is not a certain rejection (accepted, undecided, or its interval void) */
       CHAIN_R_CONFLICT = 2, /* the next move touches a contig an earlier move of its batch modified */
       CHAIN_R_PENDING = 3,  /* ... is a windowed winner without a predicted delta */
       CHAIN_R_OVERFLOW = 4, /* ... did not fit a pool / the exact kernel's grid / holds a score of exactly 0.0 */
       CHAIN_R_NO_SLOTS = 5, /* no slot scored under the model's parameters is left (batch used up, parameters promoted, first step) */
       CHAIN_R_UNSUPPORTED = 6 /* the histogram tier is not in use (its cost model, verify mode, no mapped host memory) */ };
static int ensure_chain(ig_ctx* c)
{
    if (c->chain_sets) return 0;
    DALLOC(c->chain_sets, CHAIN_MAX);
    DALLOC(c->chain_in, CHAIN_MAX);
    DALLOC(c->chain_tests, CHAIN_SEG);
    DALLOC(c->chain_out16, (size_t)CHAIN_SEG * 16);
    DALLOC(c->chain_zs, (size_t)CHAIN_SEG * 8);
    HIPCK(memset_now(c->chain_out16, 0, (size_t)CHAIN_SEG * 16 * sizeof(long long)));
    return 0;
}
static int nuis_chain_impl(ig_ctx* c, int32_t move, int32_t n_sets, float mean_kb)
{
    c->chain_done = 0;
    c->chain_reason = CHAIN_R_UNSUPPORTED;
    HIPCK(hipSetDevice(c->device));
    if (!c->nuis_spec) return fail("ig_nuis_chain_begin: no run (ig_nuis_run_begin)");
    if (c->nuis_in_flight) return fail("ig_nuis_chain_begin: a step is in flight (ig_nuis_end)");
    if (move != c->spec_move || move >= c->up_moves) return fail("ig_nuis_chain_begin: move %d, expected %d of %d", move, c->spec_move, c->up_moves);
    c->n_chain_calls++;
    auto leave = [&](int reason) {
        c->chain_reason = reason;
        c->n_chain_stops[reason]++;
        return 0;
    };
    if (ensure_host_nuis(c)) return -1;
    if (!c->host_bo || g_nuis_screen_verify || !nuis_hist_usable(c)) return leave(CHAIN_R_UNSUPPORTED);
    if (!c->spec_valid || c->spec_next >= c->spec_par_end || c->spec_base + c->spec_next != move) return leave(CHAIN_R_NO_SLOTS);
    if (ensure_chain(c) || ensure_nuis_hist(c)) return -1;
    hipStream_t st = c->stream;
    HIPCK(hipMemcpyAsync(c->chain_in, c->chain_in_host, (size_t)n_sets * sizeof(ChainIn), hipMemcpyHostToDevice, st));
    c->nh_tracking = true; /* the moves applied below are followed by the histogram (walked in behind their segment) */
    struct Untrack {
        ig_ctx* c;
        ~Untrack() { c->nh_tracking = false; }
    } untrack{c};
    if (nh_flush_pending(c)) return -1; /* the last move of the step before (walk on the side stream, the library stream waits for it) */
    c->main_drained = false;
    c->nuis_caught_up = false; /* (the segments' apply steps move the state on: whoever evaluates on tab_prev behind this call catches it up) */
    { /* tables and constants of ALL the call's sets at once (they depend on the parameters alone) */
        const int n_const = (std::max(std::max(PZ_MAX, LDS_PZ + 2), std::max((int)IG_TAB_SIZE, LDS_LGF)) + 255) / 256;
        hipLaunchKernelGGL(k_chain_prepare, dim3(n_const, n_sets), dim3(256), 0, st, c->glob, c->chain_in, mean_kb, c->chain_sets, c->lgf_tab,
                           c->score_const, c->pz_n, c->screen_const, c->chain_zs, n_sets);
    }
    int done = 0, reason = CHAIN_R_SETS;
    const PzTab pz0{c->pz_tab, c->pz_n};
    for (;;) {
        const int w0 = c->spec_next;
        /* (3 / 4 / 6 / 8 sets per segment: 16.9 / 17.5 / 17.4 / 17.8 k pairs/s at the headline shape -- the loop is bound by the host's proposals) */
        const int avail = std::min(std::min(CHAIN_SEG, n_sets - done), std::min(c->spec_par_end - w0, c->up_moves - c->spec_move));
        if (avail <= 0) {
            reason = (n_sets - done <= 0) ? CHAIN_R_SETS : CHAIN_R_NO_SLOTS;
            break;
        }
        if (!c->nh_valid) { /* (the first step of a run, or after moves outside one: from the current state's tables) */
            HIPCK(hipMemsetAsync(c->nh.bins, 0, (size_t)NH_NB * 4 * sizeof(long long), st));
            HIPCK(hipMemsetAsync(c->nh.dh, 0, ((size_t)c->nh.dh_n + 1) * sizeof(long long), st));
            HIPCK(hipMemsetAsync(c->nh.misc, 0, NH_MISC * sizeof(long long), st));
            hipLaunchKernelGGL(k_hist_build, dim3(2048), dim3(256), 0, st, c->rowptr, c->cc, c->tab, c->M, c->nh);
            c->nh_valid = true;
            c->nhs[7] += 1.0;
        }
        const int n_zero = std::min(256, std::max(32, c->M / 1024));
        /* (the zero-pixel sums on the CURRENT tables: the state "before its move" of every step of the segment up to its first
         * changing move -- tab_prev lags behind by the last changing move until the apply step catches it up itself, and the
         * histogram's walk of that move, launched behind the segment before, reads it as it is) */
        hipLaunchKernelGGL(k_chain_hist_eval, dim3(n_zero + NH_NB / 256 + NH_DH_BLOCKS, avail), dim3(256), 0, st, c->nh, c->glob, c->chain_sets + done,
                           c->score_const, c->chain_out16, c->tab, c->M, c->chain_zs, n_zero, pz0, c->chain_tests);
        flush_pending_sums(c);
        const int zcheck = decide_zcheck(c);
        const ChainArgs ca{c->chain_tests, c->chain_in, done, 1.0};
        if (fuse_commit(c, false)) { /* decisions and apply step in one launch */
            hipLaunchKernelGGL(k_chain_decide_commit, dim3(1), dim3(64 + FUSED_CW * 64), 0, st, c->glob, c->mb, c->d_results, c->spec_base, w0 + avail, w0,
                               c->dirty_buf, c->batch_out, (volatile int*)c->host_bo_dev, ++c->bo_seq, c->spec_prev_pending ? 0 : 1, c->st, c->tab,
                               c->tab_prev, c->init_prev, c->init_next, c->orientable, c->black, c->own_tag, c->own_idx, c->prev_touched, zcheck, ca);
        } else {
            hipLaunchKernelGGL(k_decide_chain, dim3(1), dim3(64), 0, st, c->glob, c->mb, c->d_results, c->spec_base, w0 + avail, w0, c->dirty_buf,
                               c->batch_out, (volatile int*)c->host_bo_dev, ++c->bo_seq, c->spec_prev_pending ? 0 : 1, zcheck, ca);
            hipLaunchKernelGGL(k_commit_batch, dim3(1), dim3(COMMIT_THREADS), 0, st, c->st, c->tab, c->tab_prev, c->glob, c->mb, c->init_prev,
                               c->init_next, c->orientable, c->black, c->own_tag, c->own_idx, c->prev_touched, c->d_results, c->spec_base, w0 + avail, w0,
                               c->batch_out, (NuisHost*)nullptr, 0);
        }
        int bo[16];
        if (wait_commit(c, bo, w0 == c->spec_par_begin, w0)) return -1;
        if (c->own_screened == 1 && w0 == c->spec_par_begin && !(bo[2] && bo[0] == w0 && bo[1] < 0)) size_exact_grid(c, bo);
        const int j = bo[0] - w0;
        if (j < 0 || j > avail) return fail("ig_nuis_chain: the decide step reported %d of %d pairs", j, avail);
        c->n_chain_segments++;
        c->n_chain_pairs += j;
        c->spec_next += j;
        c->spec_move += j;
        c->since_accept += j;
        nuis_run_length(c, false);
        done += j;
        if (j > 0) {
            c->spec_prev_pending = false;
            c->spec_slot = c->spec_next - 1;
            c->nhs[0] += j; /* evaluations of the histogram tier that decided a step, all of them rejections */
            c->nhs[1] += j;
            c->nscr[0] += j;
            c->nscr[1] += j;
            const bool moved = bo[11] != 0;
            c->last_moved = moved;
            for (int q = 0; q < j; q++) c->nh_p_changed = 0.98 * c->nh_p_changed + 0.02 * ((moved && q == j - 1) ? 1.0 : 0.0);
            if (moved) { /* the histogram follows the move before tab_prev does (here, on the library stream: the commit is still running) */
                hipLaunchKernelGGL(k_hist_walk, dim3(128), dim3(256), 0, st, c->rowptr, c->cc, c->tab_prev, c->glob, c->mb, c->spec_slot, c->nh);
                c->nhs[6] += 1.0;
            }
        }
        if (bo[10] == 5 || (bo[10] == 0 && bo[1] < 0 && j == avail)) continue; /* behind a changing move / the segment went through */
        if (bo[1] >= 0) reason = CHAIN_R_PENDING;
        else if (bo[10] == 4) reason = CHAIN_R_TEST;
        else if (bo[10] == 0) reason = CHAIN_R_CONFLICT;
        else reason = CHAIN_R_OVERFLOW;
        break;
    }
    HIPCK(hipGetLastError());
    c->nh_pending_slot = -1;
    c->chain_done = done;
    return leave(reason);
}

extern "C" int ig_nuis_chain_begin(ig_ctx* c, int32_t move, int32_t n_sets, const float* p_tests, const double* u, const double* temperature,
                                   float mean_subfrag_kb)
{
    IG_JOIN(c);
    if (n_sets < 1 || n_sets > CHAIN_MAX) return fail("ig_nuis_chain_begin: 1..%d sets (got %d)", CHAIN_MAX, n_sets);
    if (!c->chain_in_host) HIPCK(hipHostMalloc((void**)&c->chain_in_host, CHAIN_MAX * sizeof(ChainIn), hipHostMallocDefault));
    for (int k = 0; k < n_sets; k++) {
        ChainIn& ci = c->chain_in_host[k];
        memcpy(ci.p, p_tests + 8 * (size_t)k, sizeof ci.p);
        /* the step is rejected iff exp((L_test - L_move) / T) < u; on the device: (upper end of L_test) - L_move <= T (ln u - 2e-9), the
         * host's 1e-9 relative margin on u doubled and taken in the exponent (nuis_end_body); anything else is not decided there */
        const double T = temperature[k], uu = u[k];
        ci.ln_u = (T > 0.0 && uu > 0.0) ? T * (log(uu) - 2e-9) - 1e-12 * __builtin_fabs(T * log(uu)) : -IG_INF;
    }
    c->chain_busy = true;
    return nuis_defer(c, 1, move, nullptr, mean_subfrag_kb, n_sets);
}
/* 1: the chain has ended (ig_nuis_chain_end returns at once), 0: its segments are still being driven */
extern "C" int ig_nuis_chain_done(ig_ctx* c)
{
    NuisWorker* w = c->worker;
    return (!w || w->state.load(std::memory_order_acquire) != 1) ? 1 : 0;
}
extern "C" int ig_nuis_chain_end(ig_ctx* c, int32_t* n_done, int32_t* reason)
{
    const int rc_join = nuis_join(c); /* (a chain that failed on the helper thread: the handle must not stay "busy" behind its error) */
    if (!c->chain_busy) return rc_join ? -1 : fail("ig_nuis_chain_end: no chain was begun");
    c->chain_busy = false;
    *n_done = c->chain_done;
    *reason = c->chain_reason;
    return rc_join ? -1 : 0;
}
/* {calls, segments, pairs completed, ends by reason (CHAIN_R_*: 7 values)} since the handle was made */
extern "C" int ig_debug_nuis_chain_stats(ig_ctx* c, int64_t out10[10])
{
    IG_JOIN(c);
    out10[0] = c->n_chain_calls;
    out10[1] = c->n_chain_segments;
    out10[2] = c->n_chain_pairs;
    for (int q = 0; q < 7; q++) out10[3 + q] = c->n_chain_stops[q];
    return 0;
}
