/* ig_host_core.inc -- part of ig_hip.hip (one translation unit; included there in order): the handle: the helper thread of the nuisance runs, allocation and timers, ig_create / ig_destroy, the from-scratch pass's launches, window buffers, slice pool and batch buffers. */

/* ================================================================== host side */
static void free_genome_buffers(ig_ctx* c); /* ig_host_genome.inc */
static void free_map_buffers(ig_ctx* c);   /* ig_host_map.inc */
static void free_law_buffers(ig_ctx* c);   /* ig_host_law.inc */
static void free_junc_buffers(ig_ctx* c);  /* ig_host_junc.inc */
static void free_lift_buffers(ig_ctx* c);  /* ig_host_lift.inc */
static void free_join_buffers(ig_ctx* c, bool keep_snapshot); /* ig_host_join.inc */
static void free_emap_buffers(ig_ctx* c);  /* ig_host_emap.inc */
static void free_place_buffers(ig_ctx* c); /* ig_host_place.inc */
static void free_orient_buffers(ig_ctx* c); /* ig_host_orient.inc */
static void free_bal_buffers(ig_ctx* c);    /* ig_host_bal.inc */
static void free_gap_buffers(ig_ctx* c);    /* ig_host_gap.inc */
static void free_segplace_buffers(ig_ctx* c); /* ig_host_segplace.inc */
static void free_edit_buffers(ig_ctx* c);     /* ig_host_edit.inc */
static void free_cutjoin_buffers(ig_ctx* c);  /* ig_host_cutjoin.inc */
static void free_pairs_buffers(ig_ctx* c);    /* ig_host_pairs.inc */
static void free_pre_buffers(ig_ctx* c);      /* ig_host_pre.inc */
static void free_seq_buffers(ig_ctx* c);      /* ig_host_seq.inc */
static void free_text_buffers(ig_ctx* c);     /* ig_host_text.inc */
static void free_pyr_buffers(ig_ctx* c);      /* ig_host_pyr.inc */
static void flush_pending_sums(ig_ctx* c); /* behind a decisively accepted nuisance step: see k_nuis_promote */

/* ---- the launches of a run's NEXT step on a helper thread ------------------------------------------------------------------
 * Once a step's Metropolis test reads 600 KB instead of 160 MB (ig_kernels_nuis.cuh, tier 0) a (move, nuisance step) pair is
 * bound by the host: the caller's proposal arithmetic and the half-dozen launches of the next step, one after the other on one
 * thread.  ig_nuis_step_next hands the launches to this thread and returns; the caller computes its next proposal meanwhile.
 * EVERY entry point that takes a handle waits for the thread first (IG_JOIN): outside the task nothing is shared.  An error of
 * the deferred launches is reported by the entry point that waits for them.  IG_NUIS_ASYNC=0: no helper thread. */
struct NuisWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<int> state{0}; /* 0 idle, 1 a task is waiting / running, 2 quit */
    int rc = 0;
    std::string err;
    int kind = 0; /* the task: 0 ig_nuis_step_begin, 1 a chain of pairs (ig_nuis_chain_begin) */
    int move = 0;
    float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float mean_kb = 0;
    int n_sets = 0;
    std::thread::id tid;
};
static int nuis_step_begin_impl(ig_ctx* c, int32_t move, const float p_test[8], float mean_subfrag_kb);
static int g_nuis_async = 1; /* IG_NUIS_ASYNC=0: no helper thread (read where a run begins: nuis_latch_env) */
static int nuis_chain_impl(ig_ctx* c, int32_t move, int32_t n_sets, float mean_subfrag_kb);
static int nuis_join(ig_ctx* c)
{
    NuisWorker* w = c->worker;
    if (!w || std::this_thread::get_id() == w->tid) return 0;
    if (w->state.load(std::memory_order_acquire) == 1) {
        for (unsigned spin = 0; w->state.load(std::memory_order_acquire) == 1; spin++)
            if ((spin & 0x3ff) == 0x3ff) std::this_thread::yield();
    }
    if (w->rc) {
        w->rc = 0;
        return fail("%s", w->err.c_str());
    }
    return 0;
}
static void nuis_worker_main(ig_ctx* c)
{
    NuisWorker* w = c->worker;
    hipSetDevice(c->device);
    for (;;) {
        int st = w->state.load(std::memory_order_acquire);
        if (st == 0) { /* spin for a while (a step of a run is tens of microseconds away), then sleep */
            bool got = false;
            for (unsigned spin = 0; spin < 200000 && !got; spin++) got = w->state.load(std::memory_order_acquire) != 0;
            if (!got) {
                std::unique_lock<std::mutex> lk(w->mu);
                w->cv.wait(lk, [&] { return w->state.load(std::memory_order_acquire) != 0; });
            }
            continue;
        }
        if (st == 2) return;
        const int rc = w->kind == 1 ? nuis_chain_impl(c, w->move, w->n_sets, w->mean_kb) : nuis_step_begin_impl(c, w->move, w->p, w->mean_kb);
        if (rc) w->err = g_err;
        w->rc = rc;
        w->state.store(0, std::memory_order_release);
    }
}
/* kind 0: p_test = the step's test parameters; kind 1: a chain over the n_sets sets staged in chain_in_host */
static int nuis_defer(ig_ctx* c, int kind, int32_t move, const float* p_test, float mean_subfrag_kb, int n_sets)
{
    if (!g_nuis_async) return kind == 1 ? nuis_chain_impl(c, move, n_sets, mean_subfrag_kb) : nuis_step_begin_impl(c, move, p_test, mean_subfrag_kb);
    if (!c->worker) {
        c->worker = new NuisWorker();
        c->worker->th = std::thread(nuis_worker_main, c);
        c->worker->tid = c->worker->th.get_id();
    }
    NuisWorker* w = c->worker;
    if (nuis_join(c)) return -1;
    w->kind = kind;
    w->move = move;
    if (p_test) memcpy(w->p, p_test, sizeof w->p);
    w->mean_kb = mean_subfrag_kb;
    w->n_sets = n_sets;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->state.store(1, std::memory_order_release);
    }
    w->cv.notify_one();
    return 0;
}
static int nuis_defer_step_begin(ig_ctx* c, int32_t move, const float p_test[8], float mean_subfrag_kb)
{
    return nuis_defer(c, 0, move, p_test, mean_subfrag_kb, 0);
}
static void nuis_worker_stop(ig_ctx* c)
{
    NuisWorker* w = c->worker;
    if (!w) return;
    (void)nuis_join(c);
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->state.store(2, std::memory_order_release);
    }
    w->cv.notify_one();
    w->th.join();
    delete w;
    c->worker = nullptr;
}
#define IG_JOIN(c)                    \
    do {                              \
        if (nuis_join(c)) return -1;  \
    } while (0)

/* hipMemset runs on the NULL stream and returns before the fill has happened; the library's stream may be one the caller handed
 * over (ig_set_stream: torch's streams are non-blocking, i.e. NOT ordered behind the null stream) -- a fill that lands after the
 * kernels enqueued behind it wipes what they wrote.  Seen only with several handles keeping the device busy (tools/fuzz_ranks.py:
 * the first batch of a multi-rank run decided on a control block zeroed under it).  Every fill of the library waits for itself. */
static hipError_t memset_now(void* p, int value, size_t bytes)
{
    hipError_t e = hipMemset(p, value, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}
template <class T>
static int dalloc(T** p, size_t n, const char* name = "")
{
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail("hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
    /* IG_POISON_ALLOC=<byte> (tests, tools/fuzz_*.py): every device allocation starts filled with that byte instead of whatever the
     * allocator hands out (zero pages in a fresh process, another handle's leftovers in a long-lived one) -- a read of memory nobody
     * wrote shows up at once instead of after a thousand handles */
    static const int s_poison = getenv("IG_POISON_ALLOC") ? atoi(getenv("IG_POISON_ALLOC")) : -1;
    static const char* s_only = getenv("IG_POISON_ONLY"); /* ... only the buffers whose name (the DALLOC argument) contains this */
    if (s_poison >= 0 && (!s_only || strstr(name, s_only))) {
        e = hipMemset(*p, s_poison & 0xff, n * sizeof(T));
        if (e == hipSuccess) e = hipDeviceSynchronize(); /* (the fill runs on the null stream: the library's streams do not wait for it) */
        if (e != hipSuccess) return fail("hipMemset(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
    }
    return 0;
}
#define DALLOC(p, n)                     \
    do {                                 \
        if (dalloc(&(p), (n), #p)) return -1; \
    } while (0)

enum { T_GATHER = 0, T_MUTATE, T_SCORE, T_FINALIZE, T_DELTA, T_APPLY, T_POST, T_COMMIT, T_SLICE, T_ARGMAX, T_SCREEN, T_DIFF, T_PROBE, T_COUNT };
static const char* kTimerNames[T_COUNT] = {"gather", "mutate", "score", "finalize", "delta", "apply", "post", "commit", "slice", "argmax", "screen", "diff", "probe"};

struct TimedLaunch {
    ig_ctx* c;
    int id;
    hipEvent_t a, b;
    hipStream_t st;
    TimedLaunch(ig_ctx* ctx, int which, hipStream_t stream = nullptr) : c(ctx), id(which), a(nullptr), b(nullptr), st(stream ? stream : ctx->stream)
    {
        if (c->timing && !((c->timing_mask >> id) & 1u)) return;
        /* every timing_every-th launch only: an event record between two kernels of a stream costs ~6 us of idle queue */
        if (c->timing && c->timing_every > 1 && (c->timers[id].seen++ % c->timing_every) != 0) return;
        if (c->timing) { /* events are recycled (drain_timers): creating a pair costs microseconds the timed call should not pay */
            if (c->ev_pool.size() >= 2) {
                a = c->ev_pool.back();
                c->ev_pool.pop_back();
                b = c->ev_pool.back();
                c->ev_pool.pop_back();
            } else {
                hipEventCreate(&a);
                hipEventCreate(&b);
            }
            hipEventRecord(a, st);
        }
    }
    ~TimedLaunch()
    {
        if (c->timing && a) {
            hipEventRecord(b, st);
            c->timers[id].ev.emplace_back(a, b);
        }
    }
};

static void drain_timers(ig_ctx* c)
{
    for (int i = 0; i < T_COUNT; i++) {
        for (auto& pr : c->timers[i].ev) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                c->timers[i].total_ms += ms;
                c->timers[i].n++;
            }
            c->ev_pool.push_back(pr.first);
            c->ev_pool.push_back(pr.second);
        }
        c->timers[i].ev.clear();
    }
}

/* a zeroed block of pinned host memory the kernels write themselves (mapped, coherent: no copy, no stream synchronisation) and its
 * device address -- *dev stays null where the block cannot be mapped or IG_NO_HOST_FLAG=1 says not to (tests: the copying paths);
 * need_dev: without a device address the block is of no use.  nullptr: no such memory. */
static void* mapped_block(size_t bytes, void** dev, bool need_dev)
{
    const bool s_no_flag = getenv("IG_NO_HOST_FLAG") && atoi(getenv("IG_NO_HOST_FLAG")); /* (read per block: a test toggles it between handles) */
    void *hp = nullptr, *dp = nullptr;
    *dev = nullptr;
    if ((need_dev && s_no_flag) || hipHostMalloc(&hp, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) hp = nullptr;
    if (hp && !s_no_flag && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) *dev = dp;
    if (hp && need_dev && !*dev) {
        hipHostFree(hp);
        hp = nullptr;
    }
    if (hp) memset(hp, 0, bytes);
    (void)hipGetLastError();
    return hp;
}

static const double kWindowBudget = 64e9; /* ig_ctx.window_budget unless ig_debug_window_budget says otherwise (slots_in_budget) */

extern "C" const char* ig_last_error(void) { return g_err.c_str(); }

extern "C" int ig_create(int device_id, ig_ctx** out)
{
    if (!out) return fail("ig_create: out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail("ig_create: no HIP device (the MI355X path has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return fail("ig_create: device %d out of range (%d devices)", device_id, n);
    HIPCK(hipSetDevice(device_id));
    ig_ctx* c = new ig_ctx(); /* value-initialised: every field starts as zero / null / false; what follows is what does not */
    c->device = device_id;
    c->own_stream = true;
    c->world = 1;
    c->timing_mask = 0xffff;
    c->side_busy = true;
    c->timing_every = 1;
    c->window_budget = kWindowBudget;
    for (int i = 0; i < T_COUNT; i++) {
        c->timers[i].name = kTimerNames[i];
        c->timers[i].total_ms = 0;
        c->timers[i].n = 0;
    }
    c->init_links_inverse = true;
    HIPCK(hipStreamCreate(&c->stream));
    HIPCK(hipStreamCreate(&c->stream2));
    HIPCK(hipStreamCreate(&c->stream3));
    HIPCK(hipEventCreateWithFlags(&c->ev_gathered, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->ev_exact, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->ev_walk, hipEventDisableTiming));
    c->last_moved = true;
    c->nh_pending_slot = -1;
    c->nh_policy_on = true;
    c->nh_p_changed = 0.1;
    c->nuis_tier = 1;
    HIPCK(hipEventCreateWithFlags(&c->ev_slice, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    DALLOC(c->glob, 1);
    DALLOC(c->scratch8, 8);
    DALLOC(c->scratch_nuis, 8);
    HIPCK(memset_now(c->glob, 0, sizeof(Glob)));
    DALLOC(c->lgf_tab, LGF_TAB);
    /* log10(ob!) table (KA:111-124, 251-270): the 15 float-factorial constants on the host, the rest on the device */
    double small[15];
    for (int k = 0; k < 15; k++) {
        float r = 1;
        if (k < 10) {
            for (int q = 1; q <= k; q++) r = r * q;
        } else {
            r = ig_powf((float)k, (float)k, ig_tab()) * ig_expf(-(float)k, ig_tab()) * __builtin_sqrtf((float)(2 * 3.14159265358979323846 * (float)k));
        }
        small[k] = ig_log10((double)r, ig_tab());
    }
    Glob hg;
    memset(&hg, 0, sizeof hg);
    for (int k = 0; k < 15; k++) hg.lgf[k] = small[k];
    const int lb[6] = {1, 3, 5, 10, 20, 50}; /* CL:417 */
    for (int k = 0; k < 6; k++) hg.list_bounds[k] = lb[k];
    hg.slice_nb = 50 * 4;
    HIPCK(hipMemcpy(c->glob, &hg, sizeof hg, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_lgf_table, dim3((LGF_TAB + 255) / 256), dim3(256), 0, c->stream, c->lgf_tab, c->glob->lgf);
    HIPCK(hipStreamSynchronize(c->stream));
    *out = c;
    return 0;
}

/* the per-window arrays of the move buffers (strides sN / sM) */
static void free_window_buffers(MoveBuf& m)
{
    hipFree(m.Lloc);
    hipFree(m.lbloc);
    hipFree(m.slloc);
    hipFree(m.subs);
    hipFree(m.rowcnt);
    hipFree(m.rowbe);
    hipFree(m.coords);
    hipFree(m.loc);
    m.Lloc = m.lbloc = m.slloc = m.subs = m.rowcnt = nullptr;
    m.rowbe = nullptr;
    m.coords = nullptr;
    m.loc = nullptr;
    m.sN = m.sM = 0;
}
static void free_slice_pool(MoveBuf& m)
{
    hipFree(m.sl_li);
    hipFree(m.sl_lj);
    hipFree(m.sl_ob);
    hipFree(m.sl_pk);
    m.sl_li = m.sl_lj = m.sl_ob = nullptr;
    m.sl_pk = nullptr;
    m.pool_cap = 0;
}
/* one set of batch buffers */
static void free_movebuf(MoveBuf& m)
{
    free_window_buffers(m);
    free_slice_pool(m);
    hipFree(m.meta);
    hipFree(m.cmeta);
    hipFree(m.part);
    hipFree(m.scores);
    hipFree(m.slbound);
    hipFree(m.sloff);
    hipFree(m.qpart);
    hipFree(m.ctl);
    hipFree(m.sinfo);
    hipFree(m.rec);
    hipFree(m.scr);
    hipFree(m.scr_void);
    hipFree(m.scr_ub);
    hipFree(m.cont);
    hipFree(m.ident);
    hipFree(m.livecol);
    hipFree(m.work);
    hipFree(m.slot_items);
    hipFree(m.pred_list);
    hipFree(m.order);
    hipFree(m.tail_n);
    hipFree(m.tail_ent);
    memset((void*)&m, 0, sizeof m);
}
static void free_move_buffers(ig_ctx* c)
{
    free_movebuf(c->mb);
    hipFree(c->own_tag);
    hipFree(c->own_idx);
    c->own_tag = c->own_idx = nullptr;
    hipFree(c->batch_out);
    hipFree(c->dirty_buf);
    c->dirty_buf = nullptr;
    c->batch_out = nullptr;
}

extern "C" void ig_destroy(ig_ctx* c)
{
    if (!c) return;
    nuis_worker_stop(c);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->stream2);
    hipStreamDestroy(c->stream2);
    hipStreamSynchronize(c->stream3);
    hipStreamDestroy(c->stream3);
    hipEventDestroy(c->ev_gathered);
    hipEventDestroy(c->ev_main);
    hipEventDestroy(c->ev_exact);
    hipEventDestroy(c->ev_walk);
    hipFree(c->probe_scr);
    hipFree(c->probe_void);
    hipFree(c->nh.bins);
    hipFree(c->nh.dh);
    hipFree(c->nh.misc);
    hipFree(c->scratch_hist);
    hipFree(c->scratch_exact);
    hipFree(c->chain_sets);
    hipFree(c->chain_in);
    hipFree(c->chain_tests);
    hipFree(c->chain_out16);
    hipFree(c->chain_zs);
    if (c->chain_in_host) hipHostFree(c->chain_in_host);
    if (c->host_nuis) hipHostFree(c->host_nuis);
    if (c->h_stage) hipHostFree(c->h_stage);
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    hipFree(c->scratch_accept);
    hipFree(c->scratch_nuis);
    hipEventDestroy(c->ev_slice);
    hipEventDestroy(c->ev_tail);
    if (c->host_bo) hipHostFree(c->host_bo);
    if (c->host_max) hipHostFree(c->host_max);
    if (c->host_step) hipHostFree(c->host_step);
    drain_timers(c);
    free_move_buffers(c);
    free_genome_buffers(c);
    free_map_buffers(c);
    free_law_buffers(c);
    free_junc_buffers(c);
    free_lift_buffers(c);
    free_join_buffers(c, false);
    free_emap_buffers(c);
    free_place_buffers(c);
    free_orient_buffers(c);
    free_bal_buffers(c);
    free_gap_buffers(c);
    free_segplace_buffers(c);
    free_edit_buffers(c);
    free_cutjoin_buffers(c);
    free_pairs_buffers(c);
    free_pre_buffers(c);
    free_seq_buffers(c);
    free_text_buffers(c);
    free_pyr_buffers(c);
    hipFree(c->st_block);
    hipFree(c->tab.dist);
    hipFree(c->tab_prev.dist);
    hipFree(c->sub_tab);
    hipFree(c->rowptr);
    hipFree(c->cc);
    hipFree(c->crow);
    hipFree(c->tabrec);
    hipFree(c->tiled_cc);
    hipFree(c->tile_work);
    hipFree(c->tile_hist);
    hipFree(c->tile_sig);
    hipFree(c->tile_info);
    hipFree(c->tile_dyn);
    hipFree(c->tile_dyn_list);
    hipFree(c->tile_partial);
    hipFree(c->tile_partial0);
    hipFree(c->diff_const);
    hipFree(c->scratch_diff);
    hipFree(c->init_prev);
    hipFree(c->init_next);
    hipFree(c->orientable);
    hipFree(c->black);
    hipFree(c->lgf_tab);
    hipFree(c->score_const);
    hipFree(c->full_const);
    hipFree(c->screen_const);
    hipFree(c->screen_worst);
    hipFree(c->glob);
    hipFree(c->d_results);
    hipFree(c->d_frags);
    hipFree(c->d_cands);
    hipFree(c->touched_bits);
    hipFree(c->prev_touched);
    hipFree(c->pz_tab);
    hipFree(c->scratch8);
    hipFree(c->pz_tab1);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int ig_sync(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    flush_pending_sums(c);
    HIPCK(hipStreamSynchronize(c->stream));
    drain_timers(c);
    return 0;
}

extern "C" int ig_set_stream(ig_ctx* c, void* s)
{
    IG_JOIN(c);
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->own_stream) hipStreamDestroy(c->stream);
    if (s) {
        c->stream = (hipStream_t)s;
        c->own_stream = false;
    } else {
        HIPCK(hipStreamCreate(&c->stream));
        c->own_stream = true;
    }
    return 0;
}

/* the from-scratch likelihood of the non-zero pixels under tables `t` and parameter set `which` -> out[0..1] */
__global__ void k_set_par(Glob* g, int which, ig_params p, float mean_kb)
{
    g->par[which] = p;
    g->mean_kb = mean_kb;
}
static int g_full_hist = -1;
/* the from-scratch pass over all contacts under parameter set `which` -> out[0..1]; zero_out: the zero-pixel pass too
 * (-> zero_out[0..5], k_full_zero).  p_host: the set's parameters, not yet on the device (a nuisance step's test set): the
 * launches that would set them, build their tables and clear `out` (8 values) are part of the pass.
 * Returns true when the zero-pixel pass was taken care of. */
static bool launch_full_nz(ig_ctx* c, const Tables& t, int which, long long* out, PzTab pz, hipStream_t stream = nullptr,
                           long long* zero_out = nullptr, const ig_params* p_host = nullptr, float mean_kb = 0.0f)
{
    const int s_wgs = 8 * 256;
    if (!stream) stream = c->stream;
    if (g_full_hist < 0) g_full_hist = 1; /* ig_debug_set_full_hist(0): read every tile's contacts */
    const int s_hist = g_full_hist;
    const bool tiled = c->tiled_cc && c->n_tile_work > 0;
    const int n_pack = (c->M + FULL_TB - 1) / FULL_TB;
    if (p_host && tiled) {
        const int n_const = (std::max(std::max(pz.n, LDS_PZ + 2), std::max((int)IG_TAB_SIZE, LDS_LGF)) + 255) / 256;
        hipLaunchKernelGGL(k_nuis_prepare, dim3(n_pack + n_const), dim3(256), 0, stream, c->glob, which, *p_host, mean_kb, (float*)pz.v, pz.n, c->lgf_tab,
                           c->full_const, out, t, c->M, c->tabrec, c->tile_sig, FULL_TB, c->tile_dyn, n_pack);
    } else {
        if (p_host) {
            hipLaunchKernelGGL(k_set_par, dim3(1), dim3(1), 0, stream, c->glob, which, *p_host, mean_kb);
            if (pz.n > 0) hipLaunchKernelGGL(k_build_pz, dim3((pz.n + 255) / 256), dim3(256), 0, stream, c->glob, (float*)pz.v, pz.n, which);
            hipMemsetAsync(out, 0, 8 * sizeof(long long), stream);
        }
        if (c->Z <= 0) return false;
        if (tiled)
            hipLaunchKernelGGL(k_pack_tab_sig, dim3(n_pack), dim3(256), 0, stream, t, c->M, c->tabrec, c->tile_sig, FULL_TB, c->tile_dyn);
        else
            hipLaunchKernelGGL(k_pack_tab, dim3((c->M + 255) / 256), dim3(256), 0, stream, t, c->M, c->tabrec);
        /* the tables of this parameter set (k_score_list's own block is parameter set 0's) */
        hipLaunchKernelGGL(k_build_score_const, dim3((LDS_PZ + 2 + 255) / 256), dim3(256), 0, stream, c->glob, pz, c->lgf_tab, c->full_const, which);
    }
    if (tiled) {
        /* the off-diagonal tiles: summed from their count histograms where the two blocks share no contig, else put on the
         * list; in the same launch (blocks behind those of the tiles) the zero-pixel pass */
        const int per = TILE_TRANS_THREADS / 64;
        const int n_trans = (c->n_tile_info + per - 1) / per, n_zero = zero_out ? std::min(256, std::max(32, c->M / 4096)) : 0; /* the zero-pixel pass: ~4 sub-fragments per thread */
        if (n_trans + n_zero > 0)
            hipLaunchKernelGGL(k_tile_trans, dim3(n_trans + n_zero), dim3(TILE_TRANS_THREADS), 0, stream, c->tile_info, c->n_tile_info, c->tile_sig,
                               c->tile_hist, c->full_const, (TileDyn*)c->tile_dyn, c->tile_dyn_list, s_hist, c->tile_partial, n_trans, t, c->glob,
                               which, c->M, zero_out);
        /* persistent workgroups over the static items and then the list */
        /* two per CU; next to a move (the nuisance step's pass, on its own stream) one per CU: persistent workgroups that took
         * every wave slot would keep the move's kernels waiting until the pass is over (k_decide_batch: 70 instead of 12 us),
         * and the pass is bound by its arithmetic, not by its occupancy */
        const int s_grid = 512;
        const int s_grid_side = 256;
        const int grid = std::min(c->n_tile_work, (stream != c->stream && c->side_busy) ? s_grid_side : s_grid);
        if (grid > 0)
            hipLaunchKernelGGL(k_full_nz_tiled, dim3(grid), dim3(FULL_TILED_THREADS), sizeof(FullTiledLds), stream, c->tile_work, c->tiled_cc,
                               c->tabrec, t.len, c->full_const, c->lgf_tab, c->M, pz.n, out, c->n_tile_static, (TileDyn*)c->tile_dyn,
                               c->tile_dyn_list, c->tile_trace, (zero_out && c->pub_sums) ? c->pub_sums : nullptr, ++c->sums_seq, c->tile_partial,
                               n_trans);
        if (zero_out && c->pub_sums) c->nuis_pub_sums = true;
        return zero_out != nullptr;
    }
    hipLaunchKernelGGL(k_full_nz, dim3(s_wgs), dim3(256), 0, stream, c->crow, c->cc, c->tabrec, t.len, c->full_const, c->lgf_tab,
                       (long long)c->Z, pz.n, out);
    return false;
}

/* The per-window arrays are strided by the largest window the genome can produce NOW: a window is the contig of the focal
 * bin plus the contig of a candidate, so twice the longest contig (Glob.max_L / max_SL: exact after a recount, raised by
 * every committed move that changed the genome by its window's total -- a batch can at most double it) with headroom,
 * not the whole genome: 12 MB instead of 0.84 GB per slot at the headline shape.  Grown when the bound grows. */
static double window_bytes_per_slot(int capC, double sN, double sM)
{
    return (double)std::max(8, capC) * ((double)NSLOT * NDYN * sN * 4.0 + sM * NSLOT * 8.0 + 3.0 * sN * 4.0 + 2.0 * sM * 4.0);
}
/* THE slot budget: the slots whose per-window arrays fit ig_ctx.window_budget at these strides (at least one: a genome whose one slot
 * is over the budget is tried, and fails in hipMalloc if it must).  max_batch_width, window_ring and ensure_window_buffers size by it. */
static int slots_in_budget(const ig_ctx* c, int capC, double sN, double sM)
{
    return (int)std::max(1.0, std::min(c->window_budget / window_bytes_per_slot(capC, sN, sM), 1e6));
}
/* slots the per-window arrays hold now (<= MoveBuf.capW: fewer once long contigs have made a slot gigabytes; 0: none allocated) */
static int slots_held(const ig_ctx* c) { return c->mb.Lloc ? c->win_slots : 0; }
static int ensure_window_buffers(ig_ctx* c)
{
    MoveBuf& m = c->mb;
    if (!m.capC || !m.capW) return 0;
    const int need_n = std::min(c->N, std::max(2 * c->max_L, 1)), need_m = std::min(c->M, std::max(2 * c->max_SL, 1));
    const bool s_full = c->full_windows; /* strides = the whole genome */
    if (m.Lloc && (s_full ? (m.sN == c->N && m.sM == c->M) : (m.sN >= need_n && m.sM >= need_m))) return 0;
    const int sN = s_full ? c->N : std::min(c->N, std::max(256, need_n + need_n / 2));
    const int sM = s_full ? c->M : std::min(c->M, std::max(768, need_m + need_m / 2));
    HIPCK(hipStreamSynchronize(c->stream));
    free_window_buffers(m);
    /* as many physical slots as the budget holds at the NEW strides (ADVICE r5: the window rule sizes the set to its ring of up to 64
     * slots once per call, and contigs that merge during the call regrow the strides -- a late, long-contig state that fitted at 24
     * slots must shrink its ring instead of failing in hipMalloc in the middle of a call) */
    c->win_slots = std::min(m.capW, slots_in_budget(c, m.capC, sN, sM));
    const size_t C = (size_t)m.capC * c->win_slots;
    DALLOC(m.Lloc, C * sN);
    DALLOC(m.lbloc, C * sN);
    DALLOC(m.slloc, C * sN);
    DALLOC(m.subs, C * sM);
    DALLOC(m.rowcnt, C * sM);
    DALLOC(m.rowbe, C * sM);
    DALLOC(m.coords, C * sM * NSLOT);
    DALLOC(m.loc, C * NSLOT * NDYN * sN);
    m.sN = sN;
    m.sM = sM;
    return 0;
}
/* the window buffers at the strides the genome needs NOW -> the slots they hold, or -1.  Whoever sizes a launch takes its cap from this
 * call's answer, so that no width can be older than the buffers it is launched on; enqueue_score refuses anything wider (slots_held). */
static int ensure_window_slots(ig_ctx* c) { return ensure_window_buffers(c) ? -1 : slots_held(c); }
/* tests: this handle's budget (bytes <= 0: the default again); the window buffers are sized anew under it at once -> *slots: what they
 * hold now (0: no move buffers yet).  Whatever was scored ahead in them is gone. */
extern "C" int ig_debug_window_budget(ig_ctx* c, double bytes, int32_t* slots)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    c->window_budget = bytes > 0 ? bytes : kWindowBudget;
    free_window_buffers(c->mb);
    c->spec_valid = false;
    const int held = ensure_window_slots(c);
    if (slots) *slots = std::max(held, 0);
    return held < 0 ? -1 : 0;
}

/* the slice pool: room for the lists of a batch.  A slot whose lists do not fit behind the earlier ones is re-run; when
 * the FIRST slot of a batch does not fit, the host grows the pool (grow_slice_pool) and repeats the batch.  The worst case
 * of one slot is capC x Z entries (windows = the whole genome); it starts at 2 Z. */
static int alloc_slice_pool_raw(MoveBuf& m, size_t entries)
{
    if (m.packed) {
        DALLOC(m.sl_pk, entries + 8192); /* slack: k_screen's look-ahead loads run past the end of the last list */
    } else {
        DALLOC(m.sl_li, entries);
        DALLOC(m.sl_lj, entries);
        DALLOC(m.sl_ob, entries);
    }
    m.pool_cap = (long long)entries;
    return 0;
}
/* a pool of `entries`: the new one is allocated BEFORE the old one is given up, so that a failed growth leaves the handle with the
 * pool it had (and pool_cap saying so).  Where both do not fit next to each other the old one goes first; if the new size then
 * still fails the old size is allocated again. */
static int alloc_slice_pool(MoveBuf& m, size_t entries)
{
    MoveBuf old = m;
    m.sl_li = m.sl_lj = m.sl_ob = nullptr;
    m.sl_pk = nullptr;
    m.pool_cap = 0;
    if (alloc_slice_pool_raw(m, entries) == 0) {
        free_slice_pool(old);
        return 0;
    }
    (void)hipGetLastError();
    free_slice_pool(m); /* (the 12-byte form is three arrays: whatever part of them was allocated) */
    const size_t old_entries = (size_t)old.pool_cap;
    free_slice_pool(old);
    if (alloc_slice_pool_raw(m, entries) == 0) return 0;
    (void)hipGetLastError();
    free_slice_pool(m);
    if (old_entries && alloc_slice_pool_raw(m, old_entries)) {
        free_slice_pool(m);
        return fail("the slice pool could neither be grown to %zu entries nor be allocated again at %zu", entries, old_entries);
    }
    return fail("hipMalloc failed: the slice pool cannot be grown to %zu entries (it stays at %zu)", entries, old_entries);
}
static int alloc_slice_pool(ig_ctx* c, size_t entries) { return alloc_slice_pool(c->mb, entries); }
static size_t slice_pool_max(const ig_ctx* c) { return (size_t)std::max<long long>(c->Z, 1) * (size_t)std::max(c->mb.capC, 1); }
static int grow_slice_pool(ig_ctx* c)
{
    const size_t mx = slice_pool_max(c);
    if ((size_t)c->mb.pool_cap >= mx) return fail("the slice pool already holds the worst case of a move (%zu entries) and the move does not fit", mx);
    HIPCK(hipStreamSynchronize(c->stream));
    return alloc_slice_pool(c, std::min(mx, (size_t)c->mb.pool_cap * 4));
}

static int alloc_movebuf(ig_ctx* c, MoveBuf& m, int capC, int capW, int want_packed, size_t pool_entries);
static int ensure_move_buffers(ig_ctx* c, int capC, int capW = 1)
{
    const int want_packed = (!(getenv("IG_WIDE_LISTS") && atoi(getenv("IG_WIDE_LISTS"))) && c->M < (1 << 20) && c->max_count < (1 << 24)) ? 1 : 0;
    if (c->mb.capC >= capC && c->mb.capW >= capW && c->mb.N == c->N && c->mb.M == c->M && c->mb.packed == want_packed)
        return ensure_window_buffers(c);
    if (c->N == 0 || c->M == 0) return 0;
    capC = std::max(capC, c->mb.capC);
    capW = std::max(capW, c->mb.capW);
    HIPCK(hipStreamSynchronize(c->stream));
    free_move_buffers(c);
    const size_t N = c->N;
    c->mb.capC = capC; /* (slice_pool_max reads it) */
    size_t Zc = std::min(slice_pool_max(c), std::max<size_t>((size_t)1 << 22, 2 * (size_t)std::max<long long>(c->Z, 1))); /* 32 MB, or 2 Z */
    if (const char* e = getenv("IG_POOL_ENTRIES")) /* tests: a small pool forces the overflow / re-run / growth paths */
        Zc = std::max<size_t>((size_t)atoll(e), 1024);
    if (alloc_movebuf(c, c->mb, capC, capW, want_packed, Zc)) return -1;
    DALLOC(c->own_tag, N);
    DALLOC(c->own_idx, N);
    HIPCK(memset_now(c->own_tag, 0xff, N * sizeof(int)));
    DALLOC(c->batch_out, 16);
    /* the batch outcome is also written to mapped host memory (commit_loop polls it); without it: copy + synchronise */
    if (!c->host_bo) c->host_bo = (int*)mapped_block(16 * sizeof(int), (void**)&c->host_bo_dev, true);
    DALLOC(c->dirty_buf, 2 * IG_MAX_BATCH + 4);
    return ensure_window_buffers(c);
}

/* the arrays of one set of batch buffers but the per-window ones (ensure_window_buffers) */
static int alloc_movebuf(ig_ctx* c, MoveBuf& m, int capC, int capW, int want_packed, size_t pool_entries)
{
    const size_t C = (size_t)capC * capW;
    m.N = c->N;
    m.M = c->M;
    m.capC = capC;
    m.capW = capW;
    m.packed = want_packed; /* IG_WIDE_LISTS=1 (tests) forces the 12-byte form */
    m.rot = 0;
    m.wmask = 0x7fffffff;
    m.keep = 0ull;
    m.ring = 0;
    if (alloc_slice_pool(m, pool_entries)) return -1;
    DALLOC(m.slbound, C * SLICE_SEG);
    DALLOC(m.sloff, C * SLICE_SEG);
    DALLOC(m.meta, C);
    DALLOC(m.cmeta, C * NSLOT * NCODE);
    DALLOC(m.part, C * P_STRIDE);
    DALLOC(m.qpart, C * Q_STRIDE);
    DALLOC(m.scores, C * IG_N_TMP_STRUCT);
    DALLOC(m.ctl, (size_t)capW);
    DALLOC(m.sinfo, C * NSLOT);
    m.rec_stride = rec_bytes_per_slot(capC);
    DALLOC(m.rec, m.rec_stride * (size_t)capW);
    DALLOC(m.scr, C * NSLOT);
    DALLOC(m.scr_void, C);
    DALLOC(m.scr_ub, C);
    DALLOC(m.cont, C);
    DALLOC(m.ident, C);
    HIPCK(memset_now(m.ident, 0, C * sizeof(unsigned)));
    DALLOC(m.livecol, C);
    HIPCK(memset_now(m.livecol, 0, C * sizeof(unsigned)));
    m.work_cap = (int)std::min<size_t>((size_t)1 << 20, 4 * C * NSLOT * SLICE_SEG + 4096);
    DALLOC(m.work, (size_t)m.work_cap + 32);
    DALLOC(m.slot_items, (size_t)capW * 8);
    DALLOC(m.pred_list, (size_t)capW + 8);
    HIPCK(memset_now(m.pred_list, 0, ((size_t)capW + 8) * sizeof(int)));
    DALLOC(m.order, C + (size_t)capW);
    HIPCK(memset_now(m.order, 0, (C + (size_t)capW) * sizeof(int)));
    DALLOC(m.tail_n, C);
    DALLOC(m.tail_ent, C * 3 * 64);
    HIPCK(memset_now(m.tail_n, 0xff, C * sizeof(int)));
    HIPCK(memset_now(m.cont, 0xff, C * sizeof(unsigned)));
    HIPCK(memset_now(m.cmeta, 0, C * NSLOT * NCODE * sizeof(ColMeta)));
    HIPCK(memset_now(m.slbound, 0, C * SLICE_SEG * sizeof(long long)));
    m.nseg = 8;
    HIPCK(memset_now(m.ctl, 0, (size_t)capW * sizeof(MoveCtl)));
    return 0;
}
