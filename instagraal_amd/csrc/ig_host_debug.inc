/* ig_host_debug.inc -- part of ig_hip.hip (one translation unit; included there in order): timers and the debug ABI of the kernel-granularity tests. */

extern "C" int ig_kernel_time_ms(ig_ctx* c, const char* name, double* avg_ms, int64_t* n)
{
    IG_JOIN(c);
    drain_timers(c);
    for (int i = 0; i < T_COUNT; i++)
        if (!strcmp(name, c->timers[i].name)) {
            if (avg_ms) *avg_ms = c->timers[i].n ? c->timers[i].total_ms / (double)c->timers[i].n : 0.0;
            if (n) *n = c->timers[i].n;
            return 0;
        }
    return fail("ig_kernel_time_ms: unknown kernel '%s'", name);
}

extern "C" int ig_reset_timers(ig_ctx* c, int enable)
{
    IG_JOIN(c);
    HIPCK(hipStreamSynchronize(c->stream));
    drain_timers(c);
    for (int i = 0; i < T_COUNT; i++) {
        c->timers[i].total_ms = 0;
        c->timers[i].n = 0;
    }
    c->timing = enable != 0;
    c->timing_mask = enable > 1 ? (unsigned)(enable >> 1) : 0xffffu; /* enable = 1 | (mask << 1) */
    while (enable && c->ev_pool.size() < 16) { /* the first timed launches find their events ready */
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) break;
        c->ev_pool.push_back(e);
    }
    for (int i = 0; i < T_COUNT; i++) c->timers[i].seen = 0;
    return 0;
}

/* time every n-th launch of the selected kernels only (default 1: every launch) */
extern "C" int ig_set_timer_sampling(ig_ctx* c, int every)
{
    IG_JOIN(c);
    c->timing_every = std::max(1, every);
    return 0;
}

/* ------------------------------------------------------------------ debug ABI */

extern "C" int ig_debug_eval_terms(ig_ctx* c, const float* s, const float* s_tot, const int32_t* ob, int64_t n, float* ex, float* exc,
                                   double* term, int64_t* q)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->have_params) return fail("ig_debug_eval_terms: set parameters first");
    float *ds, *dst, *dex, *dexc;
    int* dob;
    double* dterm;
    long long* dq;
    DALLOC(ds, (size_t)n);
    DALLOC(dst, (size_t)n);
    DALLOC(dob, (size_t)n);
    DALLOC(dex, (size_t)n);
    DALLOC(dexc, (size_t)n);
    DALLOC(dterm, (size_t)n);
    DALLOC(dq, (size_t)n);
    HIPCK(hipMemcpy(ds, s, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(dst, s_tot, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(dob, ob, n * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_debug_terms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, ds, dst, dob, (long long)n, c->glob,
                       c->lgf_tab, dex, dexc, dterm, dq);
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(ex, dex, n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(exc, dexc, n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(term, dterm, n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(q, dq, n * sizeof(long long), hipMemcpyDeviceToHost));
    hipFree(ds);
    hipFree(dst);
    hipFree(dob);
    hipFree(dex);
    hipFree(dexc);
    hipFree(dterm);
    hipFree(dq);
    return 0;
}

extern "C" int ig_debug_candidate_state(ig_ctx* c, int32_t cand, int32_t slot, int32_t* soa)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    if (cand < 0 || cand >= c->mb.capC || slot < 0 || slot > IG_N_TMP_STRUCT) return fail("ig_debug_candidate_state: bad index");
    const size_t n = c->N;
    CandMeta m;
    HIPCK(hipMemcpy(&m, c->mb.meta + cand, sizeof m, hipMemcpyDeviceToHost));
    if (m.kidx[slot] < 0) return fail("ig_debug_candidate_state: slot %d was not materialised for candidate %d", slot, cand);
    /* start from the live genome (internal ids), overlay the local window */
    std::vector<int> host(17 * n);
    HIPCK(hipMemcpy(host.data(), c->st_block, 17 * n * sizeof(int), hipMemcpyDeviceToHost));
    const size_t sn = (size_t)c->mb.sN; /* stride of the window arrays */
    std::vector<int> loc((size_t)NDYN * sn), gid(sn);
    HIPCK(hipMemcpy(loc.data(), c->mb.loc + ((size_t)(cand * NSLOT + slot) * NDYN) * sn, (size_t)NDYN * sn * sizeof(int), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(gid.data(), c->mb.Lloc + (size_t)cand * sn, sn * sizeof(int), hipMemcpyDeviceToHost));
    for (int x = 0; x < m.n_loc; x++)
        for (int k = 0; k < NDYN; k++) host[k * n + gid[x]] = loc[k * sn + x];
    static const int dyn_src[NDYN] = {0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13};
    for (int k = 0; k < NDYN; k++) memcpy(soa + dyn_src[k] * n, &host[k * n], n * sizeof(int));
    memcpy(soa + 4 * n, &host[11 * n], n * sizeof(int));
    memcpy(soa + 5 * n, &host[12 * n], n * sizeof(int));
    memcpy(soa + 14 * n, &host[14 * n], n * sizeof(int));
    memcpy(soa + 15 * n, &host[15 * n], n * sizeof(int));
    memcpy(soa + 16 * n, &host[16 * n], n * sizeof(int));
    for (size_t f = 0; f < n; f++) soa[7 * n + f] = (int)f;
    return 0;
}

extern "C" int ig_debug_last_sums(ig_ctx* c, int64_t* nz_hi, int64_t* nz_lo, int64_t* z_hi, int64_t* z_lo, int64_t* n_intra,
                                  int64_t* ext_hi, int64_t* ext_lo, int64_t* n_slice, int32_t* n_uniq, int32_t* uniq)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    MoveCtl mc;
    HIPCK(hipMemcpy(&mc, c->mb.ctl, sizeof mc, hipMemcpyDeviceToHost));
    const int C = mc.C;
    std::vector<long long> part((size_t)C * P_STRIDE), qp((size_t)C * Q_STRIDE);
    std::vector<CandMeta> meta(C);
    HIPCK(hipMemcpy(part.data(), c->mb.part, part.size() * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(qp.data(), c->mb.qpart, qp.size() * sizeof(long long), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(meta.data(), c->mb.meta, C * sizeof(CandMeta), hipMemcpyDeviceToHost));
    for (int cc_ = 0; cc_ < C; cc_++) {
        const long long* p = &part[(size_t)cc_ * P_STRIDE];
        const long long* q = &qp[(size_t)cc_ * Q_STRIDE];
        n_uniq[cc_] = meta[cc_].n_uniq;
        n_slice[cc_] = slice_total(p);
        int64_t eh = p[P_NZ], el = p[P_NZ + 1];
        ig_acc_normalize(&eh, &el);
        ext_hi[cc_] = eh;
        ext_lo[cc_] = el;
        for (int s = 0; s < IG_N_TMP_STRUCT; s++) {
            const int o = cc_ * IG_N_TMP_STRUCT + s;
            uniq[o] = -1;
            nz_hi[o] = nz_lo[o] = z_hi[o] = z_lo[o] = n_intra[o] = 0;
        }
        for (int k = 1; k <= meta[cc_].n_uniq; k++) {
            const int s = meta[cc_].uniq[k - 1];
            const int o = cc_ * IG_N_TMP_STRUCT + s;
            uniq[cc_ * IG_N_TMP_STRUCT + (k - 1)] = s;
            int64_t h = q[Q_NZFULL + 2 * k], l = q[Q_NZFULL + 2 * k + 1];
            const int r = (int)(slice_total(p) % 64);
            if (r > 0 && (k - 1) >= r) { /* quirk Q5 */
                h -= q[Q_TAIL + 2 * k];
                l -= q[Q_TAIL + 2 * k + 1];
            }
            ig_acc_normalize(&h, &l);
            nz_hi[o] = h;
            nz_lo[o] = l;
            h = hg.z_hi + q[Q_Z + 2 * k] - q[Q_Z];
            l = hg.z_lo + q[Q_Z + 2 * k + 1] - q[Q_Z + 1];
            ig_acc_normalize(&h, &l);
            z_hi[o] = h;
            z_lo[o] = l;
            n_intra[o] = hg.n_intra + q[Q_NI + k] - q[Q_NI];
        }
    }
    return 0;
}

extern "C" int ig_debug_tables(ig_ctx* c, float* dist, int32_t* id_c, float* s_tot, int32_t* pos, int32_t* len)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    const size_t m = c->M;
    HIPCK(hipMemcpy(dist, c->tab.dist, m * 4, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(s_tot, c->tab.stot, m * 4, hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(len, c->tab.len, m * 4, hipMemcpyDeviceToHost));
    std::vector<int2> cp(m);
    HIPCK(hipMemcpy(cp.data(), c->tab.cp, m * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; i++) {
        id_c[i] = cp[i].x;
        pos[i] = cp[i].y;
    }
    return 0;
}

/* the P_z table of parameter set `which` as ig_set_params left it (k_build_pz): *n its length, out[0 .. min(*n, cap)) its entries */
extern "C" int ig_debug_pz_table(ig_ctx* c, int32_t which, float* out, int32_t cap, int32_t* n)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (which != 0 && which != 1) return fail("ig_debug_pz_table: which must be 0 or 1");
    if (!n || cap < 0 || (cap > 0 && !out)) return fail("ig_debug_pz_table: NULL argument");
    const float* tab = which == 0 ? c->pz_tab : c->pz_tab1;
    const int len = which == 0 ? c->pz_n : c->pz_n1;
    if (!tab) return fail("ig_debug_pz_table: no parameters were set for set %d", which);
    HIPCK(hipStreamSynchronize(c->stream));
    *n = len;
    const int m = std::min(len, (int)cap);
    if (m > 0) HIPCK(hipMemcpy(out, tab, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

/* v_log_f32 / v_exp_f32 over their whole domain against the contract's double functions (the screening bound assumes
 * both below SCR_KL = SCR_KE = 4 in these units): out[0], out[1] as k_transcendental_error defines them */
extern "C" int ig_debug_transcendental_error(ig_ctx* c, double out2[2])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    double* d;
    DALLOC(d, 2);
    HIPCK(hipMemsetAsync(d, 0, 2 * sizeof(double), c->stream));
    hipLaunchKernelGGL(k_transcendental_error, dim3(256 * 16), dim3(256), 0, c->stream, d);
    HIPCK(hipMemcpyAsync(out2, d, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    hipFree(d);
    return 0;
}

/* {largest |screened - exact| / bound seen, largest bound} of the runs under IG_SCREEN_VERIFY=1; {columns screened, columns
 * scored exactly} since the state was uploaded */
extern "C" int ig_debug_screen_stats(ig_ctx* c, double out4[6])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    out4[0] = out4[1] = 0.0;
    if (c->screen_worst) HIPCK(hipMemcpy(out4, c->screen_worst, 2 * sizeof(double), hipMemcpyDeviceToHost));
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    out4[2] = (double)hg.scr_cols;
    out4[3] = (double)hg.scr_cont;
    out4[4] = (double)hg.scr_terms;
    out4[5] = (double)hg.scr_terms_exact;
    return 0;
}

/* one from-scratch pass with every workgroup of k_full_nz_tiled leaving {start, end (100 MHz clock), XCC_ID << 32 | HW_ID, contacts}:
 * out [4 x n]; n_items receives the number of workgroups */
extern "C" int ig_debug_tile_trace(ig_ctx* c, int64_t* out, int64_t cap, int64_t* n_items)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    *n_items = c->n_tile_work;
    if (!out || cap < c->n_tile_work) return 0;
    long long* d = nullptr;
    DALLOC(d, (size_t)4 * c->n_tile_work);
    HIPCK(memset_now(d, 0, (size_t)32 * c->n_tile_work));
    *n_items = std::min(c->n_tile_work, 4096);
    c->tile_trace = d;
    double nz;
    const int rc = ig_full_likelihood(c, 0, 0, &nz, nullptr, nullptr);
    c->tile_trace = nullptr;
    if (!rc) HIPCK(hipMemcpy(out, d, (size_t)32 * c->n_tile_work, hipMemcpyDeviceToHost));
    hipFree(d);
    return rc;
}

/* one screened nuisance pass (csrc/ig_kernels_nuis.cuh) under test parameters p_test on the tables of the state before the last
 * move, every workgroup leaving {start, end (100 MHz clock), XCC_ID << 32 | HW_ID, items << 32 | contacts, ticks until its blocks
 * were staged, ticks in its contact loops, 0, 0}: out [8 x n]; *n receives the number of workgroups; sums8 the pass's eight output
 * words */
extern "C" int ig_debug_diff_trace(ig_ctx* c, const float p_test[8], float mean_subfrag_kb, int64_t* out, int64_t cap, int64_t* n, int64_t* sums8)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->tiled_cc || c->n_tile_work <= 0 || !c->score_const || !c->screen_const || !c->pz_tab) return fail("ig_debug_diff_trace: no tiled contacts / parameters");
    const int grid = std::min(c->n_tile_work, 512);
    *n = grid;
    if (!out || cap < grid) return 0;
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipStreamSynchronize(c->stream3));
    if (ensure_host_nuis(c)) return -1;
    if (!c->pz_tab1) DALLOC(c->pz_tab1, PZ_MAX);
    const double need = (mean_subfrag_kb > 0) ? (double)p_test[5] / (double)mean_subfrag_kb + 2.0 : 0.0;
    c->pz_n1 = (need > 0 && need < (double)PZ_MAX) ? (int)need : ((need >= (double)PZ_MAX) ? PZ_MAX : 0);
    const ig_params hp = {p_test[0], p_test[1], p_test[2], p_test[3], p_test[4], p_test[5], p_test[6], p_test[7]};
    long long* d = nullptr;
    DALLOC(d, (size_t)8 * grid);
    HIPCK(memset_now(d, 0, (size_t)64 * grid));
    c->diff_trace = d;
    const bool sb = c->side_busy;
    c->side_busy = false;
    const bool ver = g_nuis_screen_verify;
    g_nuis_screen_verify = 0;
    const int rc = launch_nuis_prepare(c, hp, mean_subfrag_kb, c->stream3, false) || launch_nuis_diff(c, hp, c->stream3, true);
    g_nuis_screen_verify = ver;
    c->side_busy = sb;
    c->diff_trace = nullptr;
    c->nuis_diff = false;
    HIPCK(hipStreamSynchronize(c->stream3));
    if (!rc) HIPCK(hipMemcpy(out, d, (size_t)64 * grid, hipMemcpyDeviceToHost));
    if (!rc && sums8) HIPCK(hipMemcpy(sums8, c->scratch_diff, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    hipFree(d);
    return rc;
}

/* seconds ig_nuis_end (also inside ig_nuis_step_next) has spent waiting for the device since the handle was created */
extern "C" int ig_debug_nuis_wait(ig_ctx* c, double* seconds)
{
    IG_JOIN(c);
    *seconds = c->nuis_wait_s;
    return 0;
}

/* the from-scratch pass with (1, default) / without (0) the count histograms of the all-trans tiles: same sums */
extern "C" int ig_debug_set_full_hist(int on)
{
    g_full_hist = on ? 1 : 0;
    return 0;
}

/* fault injection for the decide step's zero-score rule: every n-th move of a two-tier batch is treated as one whose contenders hold
 * a score of exactly 0.0 (stop code 3: the move is scored again with every column exact); 0 = off.  *fallbacks (may be NULL): how
 * often a handle has taken that path. */
extern "C" int ig_debug_set_zero_inject(int every)
{
    g_zero_inject = every > 0 ? every : 0;
    return 0;
}
extern "C" int ig_debug_zero_fallbacks(ig_ctx* c, int64_t* fallbacks)
{
    IG_JOIN(c);
    *fallbacks = c->n_zero_fallbacks;
    return 0;
}

/* the census of decide_rounds (k_decide_commit_par): with the switch on, every round adds one to the counter of the way it ended
 * (Glob.census, IG_RC_*: ig_common.cuh); off (default) the kernel tests one bit per round and counts nothing.  clear = 1 zeroes the
 * handle's counters behind the read. */
extern "C" int ig_debug_set_round_census(int on)
{
    g_round_census = on ? 1 : 0;
    return 0;
}
extern "C" int ig_debug_round_census(ig_ctx* c, int32_t* out16, int32_t clear)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(out16, c->glob->census, 16 * sizeof(int), hipMemcpyDeviceToHost));
    if (clear) HIPCK(memset_now(c->glob->census, 0, 16 * sizeof(int)));
    return 0;
}

extern "C" int ig_debug_set_tail_quirk(int on)
{
    g_tail_quirk = on;
    return 0;
}

/* maintained exact sums {nz_hi, nz_lo, z_hi, z_lo, n_intra} and {n_contigs, next_cid, ch_c, ch_k, ch_slot, ch_windowed} */
/* Glob.dbg: what raised a device-side consistency failure (and, in tuning builds, a kernel's tick counters); clear = 1 zeroes it */
extern "C" int ig_debug_dbg(ig_ctx* c, int32_t* out8, int32_t clear)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(out8, c->glob->dbg, 8 * sizeof(int), hipMemcpyDeviceToHost));
    if (clear) HIPCK(memset_now(c->glob->dbg, 0, 8 * sizeof(int)));
    return 0;
}

extern "C" int ig_debug_globals(ig_ctx* c, int64_t* sums5, int32_t* ints6)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    flush_pending_sums(c);
    HIPCK(hipStreamSynchronize(c->stream));
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    sums5[0] = hg.nz_hi;
    sums5[1] = hg.nz_lo;
    sums5[2] = hg.z_hi;
    sums5[3] = hg.z_lo;
    sums5[4] = hg.n_intra;
    ints6[0] = hg.n_contigs;
    ints6[1] = hg.next_cid;
    MoveCtl mc;
    memset(&mc, 0, sizeof mc);
    if (c->mb.ctl) HIPCK(hipMemcpy(&mc, c->mb.ctl, sizeof mc, hipMemcpyDeviceToHost));
    ints6[2] = mc.ch_c;
    ints6[3] = mc.ch_k;
    ints6[4] = mc.ch_slot;
    ints6[5] = mc.ch_windowed;

    return 0;
}

/* one-move path (ig_step, ig_score_move, ig_apply, ig_step_begin, ig_step_batch at width 1, ig_nuis_begin): moves whose lists did not
 * fit the slice pool and were repeated with a larger one, since the handle was made */
extern "C" int ig_debug_step_stats(ig_ctx* c, int64_t out2[2])
{
    IG_JOIN(c);
    out2[0] = c->step_seq;
    out2[1] = c->n_step_tail;
    return 0;
}

extern "C" int ig_debug_pool_retries(ig_ctx* c, int64_t* n)
{
    IG_JOIN(c);
    *n = c->n_pool_retries;
    return 0;
}

/* ---- the shared layers of the reports on caller data (tests/test_hip_rows_direct.py): the 64-bit scan and the row builder, both
 * unchanged.  Neither reads anything uploaded to the handle: a created handle is enough. */

static int debug_scan64_impl(ig_ctx* c, uint64_t* in, int n, int n_arrays, long long stride, uint64_t* out, unsigned long long*& d_in,
                             unsigned long long*& d_out, unsigned long long*& d_tot)
{
    const size_t words = (size_t)n_arrays * (size_t)stride;
    DALLOC(d_in, words);
    DALLOC(d_out, words);
    DALLOC(d_tot, (size_t)n_arrays * scan_chunks(n));
    HIPCK(hipMemcpyAsync(d_in, in, words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d_out, out, words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    scan64_enqueue(c, d_in, d_out, stride, n, n_arrays, d_tot);
    HIPCK(hipMemcpyAsync(out, d_out, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(in, d_in, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ig_debug_scan64(ig_ctx* c, uint64_t* in, int32_t n, int32_t n_arrays, int64_t stride, uint64_t* out)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!in || !out) return fail("ig_debug_scan64: NULL argument");
    if (n < 1 || n_arrays < 1 || n_arrays > 65535 || stride < n || stride > (1ll << 31))
        return fail("ig_debug_scan64: %d arrays of %d words, %lld apart: at least one word, at most 65535 arrays, a stride of n .. 2^31", n_arrays, n, (long long)stride);
    if (c->nuis_in_flight || c->chain_busy) return fail("ig_debug_scan64: a nuisance step or a chain is in flight");
    unsigned long long *d_in = nullptr, *d_out = nullptr, *d_tot = nullptr;
    const int rc = debug_scan64_impl(c, in, n, n_arrays, stride, out, d_in, d_out, d_tot);
    hipFree(d_in);
    hipFree(d_out);
    hipFree(d_tot);
    return rc;
}

static int debug_rows_build_impl(ig_ctx* c, const char* who, RowBuf& r, const int32_t* lo, const uint64_t* word, long long n, int U, bool reduce, bool combine,
                                 int*& d_lo, unsigned long long*& d_word, unsigned long long*& d_sc, long long forms[8], long long* n_entries, long long* n_out)
{
    DebugRows& d = c->debug_rows;
    DALLOC(d_lo, (size_t)n);
    DALLOC(d_word, (size_t)n);
    DALLOC(d_sc, 1);
    if (n > 0) {
        HIPCK(hipMemcpyAsync(d_lo, lo, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(d_word, word, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(hipMemsetAsync(d_sc, 0, sizeof(unsigned long long), c->stream));
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (n == 0) return; /* no input: nothing to launch, the rows stay empty */
        const dim3 grid(lift_blocks(n)), block(LIFT_THREADS);
        if (!scatter && combine) hipLaunchKernelGGL((k_debug_rows_emit<false, true>), grid, block, 0, c->stream, d_lo, d_word, n, slots, ent, n_ent, d_sc);
        else if (!scatter) hipLaunchKernelGGL((k_debug_rows_emit<false, false>), grid, block, 0, c->stream, d_lo, d_word, n, slots, ent, n_ent, d_sc);
        else if (combine) hipLaunchKernelGGL((k_debug_rows_emit<true, true>), grid, block, 0, c->stream, d_lo, d_word, n, slots, ent, n_ent, d_sc);
        else hipLaunchKernelGGL((k_debug_rows_emit<true, false>), grid, block, 0, c->stream, d_lo, d_word, n, slots, ent, n_ent, d_sc);
    };
    auto check = [&](long long E) { return E < 0 || E > n ? fail("%s: %lld entries of %lld (device error)", who, E, n) : 0; };
    const RowsSpec spec = {d_sc, 1, 0, 0, "", reduce, {0, 0, 0, 0, 0}};
    LiftTimer timer(c, nullptr, 0);
    unsigned long long sc[1];
    if (rows_build(c, who, r, U, spec, sc, check, emit, timer, forms, n_entries, n_out)) return -1;
    HIPCK(hipStreamSynchronize(c->stream));
    d.rowptr.assign((size_t)U + 1, 0);
    HIPCK(hipMemcpy(d.rowptr.data(), r.rowptr, ((size_t)U + 1) * sizeof(long long), hipMemcpyDeviceToHost));
    d.word.clear();
    d.col.clear();
    d.count.clear();
    if (*n_out > 0 && reduce) {
        d.col.resize((size_t)*n_out);
        d.count.resize((size_t)*n_out);
        HIPCK(hipMemcpy(d.col.data(), r.out_col, (size_t)*n_out * sizeof(int), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(d.count.data(), r.out_cnt, (size_t)*n_out * sizeof(long long), hipMemcpyDeviceToHost));
    } else if (*n_out > 0) {
        d.word.resize((size_t)*n_out);
        HIPCK(hipMemcpy(d.word.data(), r.ent, (size_t)*n_out * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    d.reduced = reduce;
    d.valid = true;
    return 0;
}

extern "C" int ig_debug_rows_build(ig_ctx* c, const int32_t* lo, const uint64_t* word, int64_t n, int32_t n_rows, int32_t reduce, int32_t combine,
                                   int64_t* n_entries, int64_t* n_out, int64_t forms[8])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_rows_build";
    c->debug_rows.valid = false; /* whatever happens, the result of an earlier build is gone */
    if (n < 0 || n_rows < 0) return fail("%s: %lld entries in %d rows: neither may be negative", who, (long long)n, n_rows);
    if (!n_entries || !n_out || !forms || (n > 0 && (!lo || !word))) return fail("%s: NULL argument", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    for (int64_t k = 0; k < n; k++) {
        if (lo[k] >= n_rows) return fail("%s: entry %lld is of row %d, there are %d rows", who, (long long)k, lo[k], n_rows);
        if (word[k] >> 63) return fail("%s: entry %lld has a column of 2^31 or more (word 0x%016llx)", who, (long long)k, (unsigned long long)word[k]);
    }
    RowBuf r;
    int* d_lo = nullptr;
    unsigned long long *d_word = nullptr, *d_sc = nullptr;
    long long f[8], E = 0, K = 0;
    const int rc = debug_rows_build_impl(c, who, r, lo, word, n, n_rows, reduce != 0, combine != 0, d_lo, d_word, d_sc, f, &E, &K);
    hipStreamSynchronize(c->stream);
    rows_free(r);
    hipFree(d_lo);
    hipFree(d_word);
    hipFree(d_sc);
    if (rc) return rc;
    for (int k = 0; k < 8; k++) forms[k] = f[k];
    *n_entries = E;
    *n_out = K;
    return 0;
}

extern "C" int ig_debug_rows_fetch(ig_ctx* c, int64_t* rowptr, int64_t n_rowptr, uint64_t* word, int32_t* col, int64_t* count, int64_t capacity)
{
    IG_JOIN(c);
    const DebugRows& d = c->debug_rows;
    if (!d.valid) return fail("ig_debug_rows_fetch: nothing is built (ig_debug_rows_build first)");
    const size_t n_out = d.reduced ? d.col.size() : d.word.size();
    if (!rowptr || n_rowptr < (int64_t)d.rowptr.size() || capacity < (int64_t)n_out)
        return fail("ig_debug_rows_fetch: the result has %zu row words and %zu entries, the caller's capacities are %lld and %lld", d.rowptr.size(), n_out,
                    (long long)n_rowptr, (long long)capacity);
    if (n_out > 0 && (d.reduced ? !col || !count : !word)) return fail("ig_debug_rows_fetch: NULL output (the result is %s)", d.reduced ? "reduced" : "not reduced");
    memcpy(rowptr, d.rowptr.data(), d.rowptr.size() * sizeof(int64_t));
    if (d.reduced && n_out > 0) {
        memcpy(col, d.col.data(), n_out * sizeof(int32_t));
        memcpy(count, d.count.data(), n_out * sizeof(int64_t));
    } else if (n_out > 0)
        memcpy(word, d.word.data(), n_out * sizeof(uint64_t));
    return 0;
}

/* ---- the wave idioms on caller data (tests/test_hip_wave_runs.py): wave_runs and wave_run_sum through k_debug_wave_runs on a bare
 * handle.  The grid is capped so that a hundred thousand entries take the grid-stride loop more than once. */
#define DEBUG_WAVE_BLOCKS 64

extern "C" int ig_debug_wave_runs(ig_ctx* c, const int32_t* keys, const int64_t* values, int64_t n, int32_t n_dest, int32_t wide, int64_t* out, int64_t* atomics)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_wave_runs";
    if (n < 0 || n_dest < 0) return fail("%s: %lld entries for %d words: neither may be negative", who, (long long)n, n_dest);
    if (!atomics || (n > 0 && (!keys || !values)) || (n_dest > 0 && !out)) return fail("%s: NULL argument", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    for (int64_t k = 0; k < n; k++)
        if (keys[k] >= n_dest) return fail("%s: entry %lld has the key %d, there are %d words", who, (long long)k, keys[k], n_dest);
    int* d_key = nullptr;
    long long* d_val = nullptr;
    unsigned long long* d_out = nullptr; /* the sums, then one word: the atomics issued */
    const int rc = [&]() -> int {
        DALLOC(d_key, (size_t)std::max<int64_t>(n, 1));
        DALLOC(d_val, (size_t)std::max<int64_t>(n, 1));
        DALLOC(d_out, (size_t)n_dest + 1);
        HIPCK(hipMemsetAsync(d_out, 0, ((size_t)n_dest + 1) * sizeof(unsigned long long), c->stream));
        if (n > 0) {
            HIPCK(hipMemcpyAsync(d_key, keys, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIPCK(hipMemcpyAsync(d_val, values, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
            const dim3 grid((unsigned)std::min<int64_t>((n + LIFT_THREADS - 1) / LIFT_THREADS, DEBUG_WAVE_BLOCKS)), block(LIFT_THREADS);
            if (wide) hipLaunchKernelGGL((k_debug_wave_runs<long long>), grid, block, 0, c->stream, d_key, d_val, (long long)n, d_out, d_out + n_dest);
            else hipLaunchKernelGGL((k_debug_wave_runs<int>), grid, block, 0, c->stream, d_key, d_val, (long long)n, d_out, d_out + n_dest);
        }
        if (n_dest > 0) HIPCK(hipMemcpyAsync(out, d_out, (size_t)n_dest * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(atomics, d_out + n_dest, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    hipStreamSynchronize(c->stream);
    hipFree(d_key);
    hipFree(d_val);
    hipFree(d_out);
    return rc;
}
