/* ig_host_batch.inc -- part of ig_hip.hip (one translation unit; included there in order): the move driver: a batch's launch sequence (enqueue_score), the decide / apply launches and their outcome, speculative batches (ig_step_batch, ig_step_batch_draw, ig_batch_*), single moves (ig_step, ig_score_move, ig_apply), contact shards. */

/* ------------------------------------------------------------------ move driver */

static int ensure_io(ig_ctx* c, int n_moves, int max_c)
{
    /* pinned staging of the lists and the result records: copies from / to the caller's pageable arrays block the host for
     * 10-20 us each, which is a tenth of a call of one batch */
    const size_t need = (size_t)n_moves * (sizeof(int) + (size_t)IG_MAX_CANDIDATES * sizeof(int) + sizeof(ig_move_result));
    if (c->h_stage_bytes < need) {
        if (c->h_stage) hipHostFree(c->h_stage);
        c->h_stage = nullptr;
        c->h_stage_bytes = 0;
        /* (at least 1 MB = 7 489 moves, and the device arrays below 8 192 moves: a pinned block is made in hundreds of microseconds and
         * hipFree waits for the device -- the driver's 480-move call behind a 120-move warm-up paid 0.6 ms of its 11 for growing all
         * five of them inside the timed region, profiles/r05final_*) */
        const size_t want = std::max(need, (size_t)1 << 20);
        if (hipHostMalloc((void**)&c->h_stage, want, hipHostMallocDefault) == hipSuccess) c->h_stage_bytes = want;
        else (void)hipGetLastError(); /* no pinned memory: the copies go through the caller's arrays */
    }
    if (c->results_cap < n_moves) {
        const int cap = std::max(n_moves, 8192);
        hipFree(c->d_results);
        hipFree(c->d_frags);
        DALLOC(c->d_results, (size_t)cap);
        DALLOC(c->d_frags, (size_t)cap);
        c->results_cap = cap;
    }
    if ((long long)c->cands_cap < (long long)n_moves * max_c) {
        const long long cap = std::max((long long)n_moves * max_c, 8192LL * IG_MAX_CANDIDATES);
        hipFree(c->d_cands);
        DALLOC(c->d_cands, (size_t)cap);
        c->cands_cap = (int)std::min(cap, (long long)0x7fffffff);
    }
    return 0;
}

static int check_ready(ig_ctx* c)
{
    if (!c->have_contacts || !c->have_sub || !c->have_state || !c->have_params)
        return fail("contacts, sub-fragment table, state and parameters must be uploaded before a move");
    flush_pending_sums(c);
    c->nuis_caught_up = false;
    c->main_drained = false;
    c->nuis_spec = c->spec_valid = false; /* every entry point that runs moves passes here: a run of ig_nuis_step_begin ends with it */
    return 0;
}

static int g_tail_quirk = 1;

/* two-tier scoring: the smallest grid of the exact kernel a batch may be launched with.  k_contend cuts a slot's work into items
 * so that the slot alone needs at most half of the grid; whatever the item size there is up to one partly filled item per
 * (candidate, column, list segment): max_c x NSLOT x SLICE_SEG of them (2 000 at 5 candidates, 6 400 at 16) */
static int exact_grid_floor(const ig_ctx* c, int max_c)
{
    return std::min(c->mb.work_cap, std::max(4096, 2 * std::max(max_c, 1) * NSLOT * std::max(c->mb.nseg, 8) + 2048));
}

/* the exact kernel's next grid from the work items the batch just decided needed (bo[6]); asked at the first commit of a scored piece */
static void size_exact_grid(ig_ctx* c, const int bo[16])
{
    c->exact_grid = std::min(c->mb.work_cap, std::max(exact_grid_floor(c, c->up_max_c), (int)(1.25 * bo[6]) + 2048));
}

/* one-move calls: the bound on the longest contig comes back with the result (the window strides follow it) */
static int queue_max_readback(ig_ctx* c)
{
    if (!c->host_max) {
        HIPCK(hipHostMalloc((void**)&c->host_max, 2 * sizeof(int), hipHostMallocDefault));
        c->host_max[0] = c->host_max[1] = 0;
    }
    HIPCK(hipMemcpyAsync(c->host_max, &c->glob->max_L, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return 0;
}
static void take_max_readback(ig_ctx* c)
{
    if (!c->host_max) return;
    c->max_L = std::max(c->max_L, c->host_max[0]);
    c->max_SL = std::max(c->max_SL, c->host_max[1]);
}

/* enqueue the scoring launches of W move slots (moves move0 .. move0+W-1 of the uploaded lists);
 * phase 0 = up to k_score_list (the sums that are all-reduced when sharded), 1 = the rest, 2 = both */
/* k_rescore_prepare: slots whose structural half (windows, candidate genomes, columns, slice lists) stands but whose
 * parameter-dependent half has to be (re)done -- the parameters changed (an accepted nuisance step), or the slots were only
 * gathered / mutated / sliced so far: accumulators back to zero, the zero-pixel sums of every column under the model's
 * current P_z table (what k_mutate left, KA:3919-4002, from the columns it wrote) */
__global__ void __launch_bounds__(256) k_rescore_prepare(Glob* g, MoveBuf mb, PzTab pz, int w_begin)
{
    const int slot = blockIdx.x, c = blockIdx.y, w = w_begin + blockIdx.z, t = threadIdx.x;
    MoveCtl& mc = mb.ctl[PS(w)];
    if (c >= mc.C) return;
    const int cw = CW(w, c);
    if (slot == 0) { /* once per candidate */
        for (int i = t; i < NSLOT * 2; i += blockDim.x) mb.part[(size_t)cw * P_STRIDE + P_NZ + i] = 0;
        for (int i = t; i < NSLOT * 2; i += blockDim.x) {
            mb.qpart[(size_t)cw * Q_STRIDE + Q_NZFULL + i] = 0;
            mb.qpart[(size_t)cw * Q_STRIDE + Q_TAIL + i] = 0;
            ((long long*)mb.scr)[(size_t)cw * NSLOT * 2 + i] = 0;
        }
        if (t == 0) {
            mb.scr_void[cw] = 0;
            mb.scr_ub[cw] = 0;
            mb.cont[cw] = 0xffffffffu;
            mb.ident[cw] = 0;
            if (c == 0) {
                mc.exact_chunk = 0;
                if (mc.overflow == 2) mc.overflow = 0; /* the exact kernel's grid is dealt out again (the slice pool's verdict, 1, stands) */
                mc.pred = -1;
                mc.pred_pad = -1;
                mc.pd_hi = mc.pd_lo = 0;
                if (blockIdx.z == 0 && mb.work)
                    for (int q = 0; q < 16; q++) mb.work[q] = 0;
            }
        }
    }
    const CandMeta& m = mb.meta[cw];
    const int k = m.kidx[slot];
    if (k < 0 || m.m_loc > mb.sM) return;
    const ig_params p = g->par[0];
    const float mean = g->mean_kb;
    const uint2* col = mb.coords + (size_t)(cw * NSLOT + k) * mb.sM;
    const ColMeta* cm = mb.cmeta + (size_t)(cw * NSLOT + k) * NCODE;
    long long hi = 0, lo = 0;
    for (int ls = t; ls < m.m_loc; ls += blockDim.x) {
        const uint2 v = col[ls];
        const int npos = (int)(v.y & 0x0fffffffu), code = (int)(v.y >> 28);
        if (npos > 0) {
            const long long q2 = zero_q(p, npos, cm[code].len, cm[code].stot, mean, pz.v, pz.n);
            hi += q2 >> 32;
            lo += (long long)(unsigned int)q2;
        }
    }
    __shared__ long long red[2][4];
    hi = wave_sum_ll(hi);
    lo = wave_sum_ll(lo);
    if ((t & 63) == 0) {
        red[0][t >> 6] = hi;
        red[1][t >> 6] = lo;
    }
    __syncthreads();
    if (t == 0) {
        long long* q = mb.qpart + (size_t)cw * Q_STRIDE;
        q[Q_Z + 2 * k] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        q[Q_Z + 2 * k + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

/* par_begin / par_end: the slots whose PARAMETER-DEPENDENT half (tail walk, screening, contenders, exact kernel, records) is
 * done by this call (default: all of [w_begin, w_end)); par_only: nothing but that half, on slots gathered, mutated and
 * sliced by an earlier call (the runs of (move, nuisance step) pairs: the structural half of a batch survives an accepted
 * step, and is scored in pieces that follow the run lengths) */
static int enqueue_score(ig_ctx* c, int move0, int W, int max_c, int force_slot, int phase, int w_begin = 0, int w_end = -1, int par_begin = -1,
                         int par_end = -1, bool par_only = false)
{
    /* the chokepoint of the slot budget: a width that did not come from the call that ensured the buffers is a host error, before any kernel */
    if (W > slots_held(c)) return fail("enqueue_score: a launch of %d slots, the window buffers hold %d (ensure_window_slots gives a launch its cap)", W, slots_held(c));
    /* slots [w_begin, w_end) are sliced and scored here (multi-GPU: the other ranks score the rest and the slot-major
     * records are all-gathered); the candidate genomes of EVERY slot are built on every rank, the commit step needs them */
    if (w_end < 0) w_end = W;
    const int nW = w_end - w_begin;
    const int pb = par_begin < 0 ? w_begin : par_begin, pe = par_end < 0 ? w_end : par_end;
    const int nWp = pe - pb;
    struct StaleGuard { /* the kernels launched below see the list of contigs modified since these slots were gathered */
        ig_ctx* c;
        StaleGuard(ig_ctx* ctx, bool on) : c(ctx) { c->mb.stale = on ? c->dirty_buf : nullptr; }
        ~StaleGuard() { c->mb.stale = nullptr; }
    } stale_guard(c, par_only && pb > 0);
    const int N = c->N;
    const int gN = std::max((N + 255) / 256, W);
    const PzTab pz{c->pz_tab, c->pz_n};
    if (phase == 0 || phase == 2) {
        const int n_tw = (c->M + 31) / 32 + 1;
        if (!par_only) {
            c->touched_flip ^= 1;
            c->mb.touched = c->touched_bits + (size_t)c->touched_flip * n_tw;
        }
        if (!par_only) { /* list segments of this batch: 16 where it is a few slots with long lists (MoveBuf.nseg) */
            const int mean_len0 = c->n_contigs_seen > 0 ? c->N / c->n_contigs_seen : 0;
            c->mb.nseg = mean_len0 >= 600 ? SLICE_SEG : 8;
        }
        if (!par_only) {
            TimedLaunch t(c, T_GATHER);
            hipLaunchKernelGGL(k_gather, dim3(gN), dim3(256), 0, c->stream, c->st, c->glob, c->mb, c->d_cands, c->d_frags, move0, W, max_c,
                               c->tab, c->tab_prev, c->prev_touched, force_slot, c->touched_bits + (size_t)(c->touched_flip ^ 1) * n_tw, n_tw);
        }
        if (!par_only) {
            TimedLaunch t(c, T_MUTATE);
            /* slots split over GPUs: only the own slots' candidate genomes are built here; k_mutate_winners rebuilds what the
             * commit step applies from the other ranks' slots */
            c->own_begin = w_begin;
            c->own_end = w_end;
            if (nW > 0) {
                /* long contigs (late in an assembly: windows of thousands of sub-fragments): more threads per candidate genome */
                const int mean_len = c->n_contigs_seen > 0 ? c->N / c->n_contigs_seen : 0;
                const int mutate_threads = mean_len >= 600 ? 1024 : (mean_len >= 150 ? 512 : 256);
                hipLaunchKernelGGL(k_mutate, dim3(NSLOT, max_c, nW), dim3(mutate_threads), 0, c->stream, c->st, c->tab, c->sub_tab, c->rowptr,
                                   c->glob, c->mb, pz, w_begin);
            }
        }
        if (force_slot < 0 && nW > 0) {
            if (!par_only) {
                TimedLaunch t(c, T_SLICE);
                hipLaunchKernelGGL(k_offsets, dim3(1), dim3(OFFSETS_THREADS), 0, c->stream, c->mb, c->glob, W, w_begin, w_end, max_c);
                /* a wave walks a row (a workgroup 4 rows at a time).  Measured at cfg3 (us per launch of 24 slots): 32 workgroups per
                 * candidate 193, 64: 156, 96: 148, 128: 136, 256 with the chunks of a row dealt to several waves: 146 */
                /* ... and with the lists in 8 segments (round 3), workgroups per plane -> moves/s: cfg3 24: 43.1 k, 32: 44.2, 40: 45.5, 48: 45.2 - 45.7,
                 * 64: 45.4, 80: 45.3, 96: 44.6, 128: 43.9; cfg2 32: 57.3 k, 48: 55.9, 96: 55.5; cfg5 32: 28.4 k, 48: 29.9, 96: 30.1; bigctg 32: 5.3 k,
                 * 48: 5.75, 96: 5.93 -- the count follows the contacts a plane holds (two contigs' rows: 2 Z / contigs of the last batch);
                 * those sweeps predate the shared walks of k_slice (every touched contig once per slot: the planes of a slot now share the rows of
                 * 3.7 contigs instead of 6 at cfg3); SLICE_RB_CONTACTS has not been swept again since */
                const int rb_auto = c->n_contigs_seen > 0
                                        ? std::min(SLICE_RB, std::max(32, (int)(2.0 * (double)c->Z / (double)c->n_contigs_seen / SLICE_RB_CONTACTS)))
                                        : SLICE_RB;
                /* (a batch of ONE -- ig_step_draw -- is six planes: 32 - 96 workgroups each leave most of the 256 CUs idle and a long row
                 * to one wave.  Workgroups per plane at that width -> median of a call at cfg3: auto 147 us, 96: 146, 192: 143, 384: 144) */
                const int rb = nW == 1 ? std::max(rb_auto, 192) : rb_auto;
                const int s_maxj = 1 << 20;
                if (c->mb.packed)
                    hipLaunchKernelGGL(k_slice<true>, dim3(rb, max_c + 1, nW), dim3(256), 0, c->stream, c->rowptr, c->cc, c->tab, c->glob, c->mb, c->rank,
                                       c->world, w_begin, s_maxj);
                else
                    hipLaunchKernelGGL(k_slice<false>, dim3(rb, max_c + 1, nW), dim3(256), 0, c->stream, c->rowptr, c->cc, c->tab, c->glob, c->mb, c->rank,
                                       c->world, w_begin, s_maxj);
            }
            if (par_only && nWp > 0)
                hipLaunchKernelGGL(k_rescore_prepare, dim3(NSLOT, max_c, nWp), dim3(256), 0, c->stream, c->glob, c->mb, pz, pb);
            if (nWp > 0) {
            /* two-tier scoring (batches on one handle, packed lists): every column through the float screening kernel, the exact
             * kernel only for the columns that can still win (ig_kernels_screen.cuh).  IG_SCREEN=0: everything exact;
             * IG_SCREEN_VERIFY=1: everything exact AND screened, the bound checked column by column. */
            const int s_screen = getenv("IG_SCREEN") ? atoi(getenv("IG_SCREEN")) : 1; /* read per launch, like the next one */
            const int verify = getenv("IG_SCREEN_VERIFY") ? atoi(getenv("IG_SCREEN_VERIFY")) : 0; /* read per launch: a test toggles it */
            /* exact_next: the decide step met a score of exactly 0.0 among the contenders (stop code 3) -- this scoring is exact in every column */
            const bool exact_once = c->exact_next && !par_only;
            if (exact_once) c->exact_next = false;
            /* (a batch of ONE is screened only for ig_step_draw without scores: every other one-move caller reads all C x 24 of them) */
            const bool screen = (s_screen || verify) && phase == 2 && (W > 1 || c->screen_w1) && c->world == 1 && c->mb.packed && !exact_once;
            /* the Q5 tail walk only needs the slice: in the screening kernel's launch (k_screen_tail), else on a second stream
             * next to k_score_list */
            c->tail_fused = screen;
            if (phase == 2 && !c->tail_fused) {
                hipEventRecord(c->ev_slice, c->stream);
                hipStreamWaitEvent(c->stream2, c->ev_slice, 0);
                hipLaunchKernelGGL(k_tail, dim3(max_c, nWp), dim3(256), 0, c->stream2, c->rowptr, c->cc, c->tab, c->glob, c->mb, c->lgf_tab,
                                   g_tail_quirk, pz, pb);
                hipEventRecord(c->ev_tail, c->stream2);
            }
            int contenders_only = 0;
            if (screen) {
                const int ny = (NSLOT + 1) / 2;
                /* the long lists first (MoveBuf.order, k_offsets): when this launch screens the slots that one placed */
                const int use_order = (!par_only && pb == w_begin && pe == w_end && nWp * max_c <= (int)OFFSETS_THREADS) ? 1 : 0;
                /* narrow batches (late in an assembly: few long contigs, a conflict at nearly every move): few (segment, pair,
                 * candidate) triples, each with a long list -- Q workgroups split a segment so that the launch has ~7 000 of them */
                const int nseg = c->mb.nseg;
                const int Q = std::max(1, std::min(8, (7000 + nseg * ny * max_c * nWp - 1) / (nseg * ny * max_c * nWp)));
                {
                    TimedLaunch t(c, T_SCREEN);
                    /* (a launch of one slot -- one move per call --: six tail workgroups per candidate, four columns each) */
                    const int tsplit = (nWp == 1 && !par_only) ? 6 : 1; /* (a re-scored slot reads its cached tail entries: one workgroup) */
                    if (c->tail_fused)
                        hipLaunchKernelGGL(k_screen_tail, dim3(max_c * nWp * tsplit + nseg * Q * ny * max_c * nWp), dim3(SCORE_THREADS), 0, c->stream,
                                           c->screen_const, c->mb, c->mb.scr, c->mb.scr_void, c->mb.scr_ub, max_c, pb, max_c * nWp * tsplit, c->rowptr, c->cc,
                                           c->tab, c->glob, c->lgf_tab, g_tail_quirk, pz, use_order, Q, tsplit);
                    else
                        hipLaunchKernelGGL(k_screen<0>, dim3(nseg * Q, ny, max_c * nWp), dim3(SCORE_THREADS), 0, c->stream, c->screen_const,
                                           c->mb, c->mb.scr, c->mb.scr_void, c->mb.scr_ub, max_c, pb, use_order, Q);
                }
                /* IG_SCREEN_PROBE=mask (tools/screen_probe.py): the screening kernel WITHOUT the parts in the mask, launched behind the real
                 * one on the same lists and columns, sums into scratch words: timed as "probe" (ig_kernel_time_ms), results untouched */
#ifdef IG_SCREEN_PROBES /* (tuning builds only: -DIG_SCREEN_PROBES, loaded through IG_DEBUG_TUNING=1 IG_HIP_LIB=...; tools/screen_probe.py) */
                static const int s_probe = getenv("IG_SCREEN_PROBE") ? atoi(getenv("IG_SCREEN_PROBE")) : -1;
                if (s_probe >= 0) {
                    const size_t C = (size_t)c->mb.capC * c->mb.capW;
                    if (!c->probe_scr) {
                        if (dalloc(&c->probe_scr, C * NSLOT) || dalloc(&c->probe_void, 2 * C)) return -1;
                    }
                    hipMemsetAsync(c->probe_scr, 0, C * NSLOT * sizeof(ScreenSum), c->stream);
                    hipMemsetAsync(c->probe_void, 0, 2 * C * sizeof(unsigned), c->stream);
                    TimedLaunch tp(c, T_PROBE);
                    const dim3 grid(nseg * Q, ny, max_c * nWp);
#define IG_PROBE(A)                                                                                                                                   \
    hipLaunchKernelGGL(k_screen<A>, grid, dim3(SCORE_THREADS), 0, c->stream, c->screen_const, c->mb, c->probe_scr, c->probe_void, c->probe_void + C, \
                       max_c, pb, use_order, Q)
                    switch (s_probe) {
                    case 1: IG_PROBE(1); break;
                    case 2: IG_PROBE(2); break;
                    case 3: IG_PROBE(3); break;
                    case 4: IG_PROBE(4); break;
                    case 5: IG_PROBE(5); break;
                    case 6: IG_PROBE(6); break;
                    case 7: IG_PROBE(7); break;
                    case 8: IG_PROBE(8); break;
                    case 16: IG_PROBE(16); break;
                    case 32: IG_PROBE(32); break;
                    case 512: IG_PROBE(512); break;
                    case 1024: IG_PROBE(1024); break;
                    case 2048: IG_PROBE(2048); break;
                    case 1032: IG_PROBE(1032); break; /* 1024 + 8 */
                    case 1544: IG_PROBE(1544); break; /* 1024 + 512 + 8 */
                    case 8192: IG_PROBE(8192); break;
                    case 8199: IG_PROBE(8199); break; /* 8192 + 7 */
                    case 4096: IG_PROBE(4096); break;
                    case 1056: IG_PROBE(1056); break; /* 1024 + 32 */
                    case 96: IG_PROBE(96); break;   /* 32 + 64 */
                    case 160: IG_PROBE(160); break; /* 32 + 128 */
                    case 288: IG_PROBE(288); break; /* 32 + 256 */
                    case 480: IG_PROBE(480); break; /* 32 + 64 + 128 + 256 */
                    default: IG_PROBE(0); break;
                    }
#undef IG_PROBE
                }
#endif
                if (c->exact_grid <= 0) c->exact_grid = 32768;
                c->exact_grid = std::max(std::min(c->exact_grid, c->mb.work_cap), exact_grid_floor(c, max_c));
                if (!c->tail_fused) hipStreamWaitEvent(c->stream, c->ev_tail, 0); /* the contender test reads the exact tail sums (quirk Q5) */
                flush_pending_sums(c); /* ... and the maintained sum (its intervals are placed with it) */
                /* (one slot: its work list from k_contend itself -- nothing lies in front of it, and the call waits for every launch) */
                hipLaunchKernelGGL(k_contend, dim3(nWp), dim3(256), 0, c->stream, c->glob, c->mb, c->mb.scr, c->mb.scr_void, c->mb.scr_ub, c->mb.cont, pb,
                                   0, c->exact_grid, EXACT_CHUNK, nWp == 1 ? 1 : 0);
                if (nWp > 1) hipLaunchKernelGGL(k_worklist, dim3(nWp), dim3(256), 0, c->stream, c->mb, c->mb.cont, pb, c->exact_grid);
                contenders_only = verify ? 0 : 1;
            }
            c->own_screened = screen ? (verify ? 2 : 1) : 0;
            TimedLaunch t(c, T_SCORE);
            const int s_eb = c->mb.nseg; /* one workgroup per (segment, column, candidate) */
            const int s_abl = getenv("IG_ABLATE") ? atoi(getenv("IG_ABLATE")) : 0; /* read per launch: a test toggles it */
            if (contenders_only) {
                /* the work list k_contend left; the grid follows what the previous batches needed (commit_loop), the workgroups
                 * past the end of the list leave on their first load, a slot whose items do not fit is re-run */
                hipLaunchKernelGGL(k_score_list<LDS_COL_SMALL>, dim3(c->exact_grid), dim3(SCORE_THREADS), 0, c->stream, c->score_const, c->mb,
                                   c->lgf_tab, pz, s_abl, max_c, pb, 1);
            } else {
                hipLaunchKernelGGL(k_score_list<LDS_COL_SMALL>, dim3(s_eb, NSLOT, max_c * nWp), dim3(SCORE_THREADS), 0, c->stream, c->score_const,
                                   c->mb, c->lgf_tab, pz, s_abl, max_c, pb, 0);
            }
            if (screen && verify) {
                if (!c->screen_worst) {
                    if (dalloc(&c->screen_worst, 2) == 0) hipMemsetAsync(c->screen_worst, 0, 2 * sizeof(double), c->stream);
                }
                hipLaunchKernelGGL(k_screen_verify, dim3(nWp), dim3(256), 0, c->stream, c->glob, c->mb, c->mb.scr, c->mb.scr_void, c->mb.scr_ub, pb,
                                   c->screen_worst);
            }
            }
        }
    }
    if (phase == 1 || phase == 2) {
        flush_pending_sums(c); /* (k_predict reads the maintained sum: with or without the screening tier in front of it) */
        if (force_slot < 0 && nWp > 0) {
            if (phase == 1) /* after the all-reduce of the list lengths (contact shards): no overlap */
                hipLaunchKernelGGL(k_tail, dim3(max_c, nWp), dim3(256), 0, c->stream, c->rowptr, c->cc, c->tab, c->glob, c->mb, c->lgf_tab,
                                   g_tail_quirk, pz, pb);
            else if (!c->tail_fused)
                hipStreamWaitEvent(c->stream, c->ev_tail, 0);
            TimedLaunch t(c, T_FINALIZE);
            hipLaunchKernelGGL(k_records, dim3(max_c, nWp), dim3(64), 0, c->stream, c->mb, pb, c->own_screened ? 1 : 0);
            /* batches: predicted windowed winners get their exact delta now (not those decided one move per call, ig_nuis_step_begin:
             * a pause costs them nothing they would not wait for anyway) */
            if (phase == 2 && W > 1 && c->world == 1 && !c->no_predict) {
                /* (windowed winners that change the genome are ~3 % of the moves: one or two of a chain's slots.  k_delta's grid used to
                 * cover every slot -- 128 x 2 x 36 workgroups of which 9 000 left on their first load, 22 us per chain; now the positions
                 * k_predict lists, at most eight: a ninth prediction is simply not made) */
                const int zcap = std::min(nWp, 8);
                /* (fewer workgroups per position -- 37 for cfg3's 300-row windows instead of DELTA_RB = 128 -- measured: 29 us instead of 17) */
                hipLaunchKernelGGL(k_predict, dim3(nWp), dim3(256), 0, c->stream, c->glob, c->mb, pb, zcap);
                hipLaunchKernelGGL(k_delta, dim3(DELTA_RB, 2, zcap), dim3(SCORE_THREADS), 0, c->stream, c->rowptr, c->cc, c->tab, c->tab_prev,
                                   c->prev_touched, c->glob, c->mb, c->lgf_tab, pz, pb, 1, 0);
            }
        }
    }
    return 0;
}

/* scores + argmax of slot w (or the forced choice of ig_apply) */
static void enqueue_choose(ig_ctx* c, int w, int force_slot)
{
    TimedLaunch t(c, T_ARGMAX);
    if (force_slot < 0) hipLaunchKernelGGL(k_scores, dim3(1), dim3(256), 0, c->stream, c->glob, c->mb, w);
    else hipLaunchKernelGGL(k_force_choice, dim3(1), dim3(1), 0, c->stream, c->glob, c->mb, force_slot);
}

/* one-move tail: exact delta, apply, genome distance, result record */
/* a move is about to be applied outside a run of (move, nuisance step) pairs: the histogram of the screened pass's first tier
 * (NuisHist) does not follow it */
static inline void nh_untracked_move(ig_ctx* c)
{
    if (!c->nh_tracking) {
        c->nh_valid = false;
        c->nh_pending_slot = -1;
    }
}

static void enqueue_apply(ig_ctx* c, int move, int w, int forced, bool log_dirty = false)
{
    nh_untracked_move(c);
    const int N = c->N;
    const PzTab pz{c->pz_tab, c->pz_n};
    {
        TimedLaunch t(c, T_DELTA);
        hipLaunchKernelGGL(k_delta, dim3(DELTA_RB, 2, 1), dim3(SCORE_THREADS), 0, c->stream, c->rowptr, c->cc, c->tab, c->tab_prev,
                           c->prev_touched, c->glob, c->mb, c->lgf_tab, pz, w, 0, 0);
    }
    {
        TimedLaunch t(c, T_APPLY);
        hipLaunchKernelGGL(k_apply, dim3(64), dim3(256), 0, c->stream, c->st, c->tab, c->glob, c->mb, w, forced, c->prev_touched);
    }
    {
        TimedLaunch t(c, T_POST);
        hipLaunchKernelGGL(k_post, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->st, c->init_prev, c->init_next, c->orientable,
                           c->black, c->glob, N);
    }
    {
        TimedLaunch t(c, T_COMMIT);
        hipLaunchKernelGGL(k_commit, dim3(1), dim3(1), 0, c->stream, c->glob, c->mb, c->d_results, move, w, log_dirty ? c->dirty_buf : (int*)nullptr,
                           c->pub_step, c->step_seq);
    }
}

static int enqueue_move(ig_ctx* c, int move, int max_c, int force_slot, int phase)
{
    if (enqueue_score(c, move, 1, max_c, force_slot, phase)) return -1;
    if (phase == 1 || phase == 2) enqueue_choose(c, 0, force_slot);
    return 0;
}

static int validate_move(ig_ctx* c, int frag_a, const int32_t* cands, int C)
{
    if (C < 1 || C > IG_MAX_CANDIDATES) return fail("a move needs 1..%d candidates (got %d)", IG_MAX_CANDIDATES, C);
    if (frag_a < 0 || frag_a >= c->N) return fail("fragment %d out of range", frag_a);
    for (int i = 0; i < C; i++) {
        if (cands[i] < 0 || cands[i] >= c->N) return fail("candidate %d out of range", cands[i]);
        if (cands[i] == frag_a)
            return fail("candidate == focal fragment (%d): the reference reads stale buffers here (quirk Q13), not supported", frag_a);
    }
    return 0;
}

static int g_zero_inject = 0; /* ig_debug_set_zero_inject: the decide step treats every n-th move of a two-tier batch as one with a score of exactly 0.0 */
static int g_round_census = 0; /* ig_debug_set_round_census: decide_rounds counts how each of its rounds ended (Glob.census) */

/* bit 0: contender-only records (two-tier scoring): the decide step checks for scores of exactly 0.0 (decide_body, stop code 3); bit 1: the
 * census of decide_rounds; bits 8 and up: the injection period */
static int decide_zcheck(const ig_ctx* c) { return (c->own_screened == 1 ? 1 : 0) | (g_round_census ? 2 : 0) | (std::max(g_zero_inject, 0) << 8); }

/* decide and apply in ONE launch (k_decide_commit: seven waves work behind the decide wave)?  0: no, 1: where that pays, 2: IG_FUSED_COMMIT=2
 * says always (and keeps decide_body's one wave: the tests compare all three; =0: never).  It pays for plain batches of moves on windows that
 * 448 threads apply as fast as k_commit_batch's 1 024 -- not for a run's one-move launches (their host waits for the record, which the
 * fused kernel writes behind a longer prologue: 10.2 k instead of 10.7 k; ig_step_draw publishes from the fused kernel: one launch less on
 * the call's critical path), not for the late shapes (bigctg: 5.7 k instead of 5.9 k).  launch_commit and the chains' driver ask here. */
static int fuse_commit(const ig_ctx* c, bool publish)
{
    static const int s_fused = getenv("IG_FUSED_COMMIT") ? atoi(getenv("IG_FUSED_COMMIT")) : 1;
    return s_fused >= 2 ? 2 : ((s_fused == 1 && (!publish || c->pub_step) && c->max_SL <= 4096) ? 1 : 0);
}

/* commit the scored batch [move0, move0 + w_now): k_commit_batch, the one-move tail for a windowed winner, resume */
/* the decide + apply launches of the slots [next, w_now) of the batch at move `done`; fused (fuse_commit) unless this is a rank's share of a
 * batch (the winners of the other ranks are mutated in between) */
static void launch_commit(ig_ctx* c, int done, int w_now, int next, int resumed_plain, bool publish = false)
{
    nh_untracked_move(c);
    flush_pending_sums(c);
    TimedLaunch t(c, T_COMMIT);
    const int fuse = fuse_commit(c, publish), zcheck = decide_zcheck(c);
    /* the decisions in rounds of DPAR moves side by side (decide_rounds, round 6) where the launch is a plain chain: moves of at most five
     * candidates (two score records per lane), nothing published to the host from inside the kernel (ig_step_draw's scores and record), at
     * least a round's worth of decisions.  IG_FUSED_COMMIT=2 keeps decide_body's one wave (the tests compare all three) */
    if (fuse == 1 && !publish && !c->pub_scores && c->up_max_c <= 5 && w_now - next >= DPAR && !(c->own_begin > 0 || c->own_end < w_now)) {
        const int seq = ++c->bo_seq;
        hipLaunchKernelGGL(k_decide_commit_par, dim3(1), dim3(DPAR * 64 + DPAR_CW * 64), 0, c->stream, c->glob, c->mb, c->d_results, done, w_now, next,
                           c->dirty_buf, c->batch_out, (volatile int*)c->host_bo_dev, seq, resumed_plain, c->st, c->tab, c->tab_prev, c->init_prev,
                           c->init_next, c->orientable, c->black, c->own_tag, c->own_idx, c->prev_touched, zcheck);
        return;
    }
    if (fuse && !(c->own_begin > 0 || c->own_end < w_now)) {
        const int seq = ++c->bo_seq;
        hipLaunchKernelGGL(k_decide_commit, dim3(1), dim3(64 + FUSED_CW * 64), 0, c->stream, c->glob, c->mb, c->d_results, done, w_now, next, c->dirty_buf,
                           c->batch_out, (volatile int*)c->host_bo_dev, seq, resumed_plain, c->st, c->tab, c->tab_prev, c->init_prev, c->init_next,
                           c->orientable, c->black, c->own_tag, c->own_idx, c->prev_touched, publish ? c->host_nuis_dev : nullptr,
                           publish ? ++c->res_seq : 0, zcheck, c->pub_scores);
        return;
    }
    hipLaunchKernelGGL(k_decide_batch, dim3(1), dim3(64), 0, c->stream, c->glob, c->mb, c->d_results, done, w_now, next, c->dirty_buf,
                       c->batch_out, (volatile int*)c->host_bo_dev, ++c->bo_seq, resumed_plain, zcheck, c->pub_scores);
    if (c->own_begin > 0 || c->own_end < w_now)
        hipLaunchKernelGGL(k_mutate_winners, dim3(2, w_now), dim3(256), 0, c->stream, c->st, c->tab, c->sub_tab, c->rowptr, c->glob,
                           c->mb, PzTab{c->pz_tab, c->pz_n}, next, c->own_begin, c->own_end, c->batch_out);
    hipLaunchKernelGGL(k_commit_batch, dim3(1), dim3(COMMIT_THREADS), 0, c->stream, c->st, c->tab, c->tab_prev, c->glob, c->mb,
                       c->init_prev, c->init_next, c->orientable, c->black, c->own_tag, c->own_idx, c->prev_touched, c->d_results, done,
                       w_now, next, c->batch_out, publish ? c->host_nuis_dev : nullptr, publish ? ++c->res_seq : 0);
}

/* what the last k_decide_batch launch reported (batch_out[0..12)), as soon as it is there: the kernel writes a copy to mapped,
 * coherent host memory; the host spins on it, every so often makes sure the stream is still alive (a fault must not hang
 * the host) and falls back to the device copy when the stream has drained without the flag */
static int wait_commit(ig_ctx* c, int bo[16], bool first_of_batch, int next)
{
    if (c->host_bo) {
        volatile int* hb = c->host_bo;
        bool got = false;
        for (unsigned spin = 0; !got; spin++) {
            if (hb[7] == c->bo_seq) {
                got = true;
            } else if ((spin & 0xfff) == 0xfff) {
                const hipError_t q = hipStreamQuery(c->stream);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) return fail("batch commit failed: %s", hipGetErrorString(q));
            }
        }
        if (got) {
            std::atomic_thread_fence(std::memory_order_acquire);
            for (int i = 0; i < 16; i++) bo[i] = hb[i];
        } else {
            HIPCK(hipMemcpy(bo, c->batch_out, 16 * sizeof(int), hipMemcpyDeviceToHost));
        }
    } else {
        HIPCK(hipMemcpyAsync(bo, c->batch_out, 16 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    if (first_of_batch) c->n_batches++;
    c->n_batch_committed += bo[0] - next;
    c->n_batch_predicted += bo[4];
    c->n_contigs_seen = bo[5];
    c->max_L = std::max(c->max_L, bo[8]);
    c->max_SL = std::max(c->max_SL, bo[9]);
    c->last_stop = bo[10];
    c->last_stale = (unsigned long long)(unsigned)bo[12] | ((unsigned long long)(unsigned)bo[13] << 32);
    if (bo[10] == 3) { /* a scored column came out as exactly 0.0 under the live scalars: the next scoring is exact in every column */
        c->exact_next = true;
        c->n_zero_fallbacks++;
    }
    return 0;
}

static int commit_loop(ig_ctx* c, int done, int w_now, int* next_out, bool publish = false)
{
    int next = 0; /* slots [0, next) of this batch are committed */
    for (;;) {
        launch_commit(c, done, w_now, next, 0, publish);
        int bo[16];
        if (wait_commit(c, bo, next == 0, next)) return -1;
        if (bo[2] && next == 0 && bo[0] == 0 && bo[1] < 0) { /* the batch's first slot did not fit the slice pool (1) or the exact
                                                               * kernel's grid (2): the caller enlarges it and repeats the batch; (3) a
                                                               * score of exactly 0.0: the caller repeats it, every column exact */
            *next_out = -bo[2];
            return 0;
        }
        if (c->own_screened == 1 && next == 0) /* first commit of this batch: size the exact kernel's next grid */
            size_exact_grid(c, bo);
        next = bo[0];
        if (bo[1] >= 0) { /* slot bo[1] chose a windowed winner: delta + apply with the one-move kernels, then go on */
            enqueue_apply(c, done + bo[1], bo[1], 0);
            c->n_batch_pending++;
            next = bo[1] + 1;
            if (next < w_now) continue;
        }
        break;
    }
    if (next == 0) {
        Glob hg;
        HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
        return fail("device-side consistency failure %d in a batch at move %d [%d %d %d %d %d %d %d %d]", hg.error, done, hg.dbg[0], hg.dbg[1], hg.dbg[2],
                    hg.dbg[3], hg.dbg[4], hg.dbg[5], hg.dbg[6], hg.dbg[7]);
    }
    *next_out = next;
    return 0;
}

static int g_batch_w = -1; /* moves scored per launch in ig_step_batch: env IG_BATCH_W, default 24; 1 = one move at a time */

/* the widest batch of moves of max_c candidates: what the slot budget holds at the strides the present contig lengths ask for (three times
 * the longest contig, at most the genome: what ensure_window_buffers allocates when it has to) */
static int max_batch_width(ig_ctx* c, int max_c)
{
    const double sN = std::min<double>(c->N, std::max(256.0, 3.0 * c->max_L)), sM = std::min<double>(c->M, std::max(768.0, 3.0 * c->max_SL));
    return std::min(slots_in_budget(c, std::max(max_c, c->mb.capC), sN, sM), IG_MAX_BATCH);
}
/* ... as ig_batch_max_width / ig_batch_upload promise it to a caller that sizes its own launches: no more than the buffers in place hold
 * where they hold fewer slots than they were asked for (strides never shrink; ig_debug_window_budget) -- the next ensure_window_slots gives
 * these or the ones above, so ig_batch_score does not refuse a width promised here */
static int promised_width(ig_ctx* c, int max_c)
{
    const int fit = max_batch_width(c, max_c), held = slots_held(c);
    return (held > 0 && held < c->mb.capW) ? std::min(fit, held) : fit;
}

static int batch_width(ig_ctx* c, int max_c)
{
    if (g_batch_w < 0) {
        const char* e = getenv("IG_BATCH_W");
        g_batch_w = e ? atoi(e) : 24;
        g_batch_w = std::min(std::max(g_batch_w, 1), IG_MAX_BATCH);
    }
    return std::min(g_batch_w, max_batch_width(c, max_c));
}

extern "C" int ig_batch_max_width(ig_ctx* c, int32_t max_c) { IG_JOIN(c); return promised_width(c, max_c); }

/* validate and upload the pre-drawn (fragment, candidates) lists of a run of moves */
static int upload_moves(ig_ctx* c, int n_moves, const int32_t* frags, const int32_t* cands, int max_c)
{
    if (max_c < 1 || max_c > IG_MAX_CANDIDATES) return fail("max_c out of range");
    for (int i = 0; i < n_moves; i++) {
        int C = 0;
        while (C < max_c && cands[(size_t)i * max_c + C] >= 0) C++;
        for (int k = C; k < max_c; k++)
            if (cands[(size_t)i * max_c + k] >= 0) return fail("candidates must be packed before the -1 padding");
        if (validate_move(c, frags[i], cands + (size_t)i * max_c, C)) return -1;
    }
    if (ensure_io(c, n_moves, max_c)) return -1;
    HIPCK(hipMemcpyAsync(c->d_frags, frags, (size_t)n_moves * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(c->d_cands, cands, (size_t)n_moves * max_c * sizeof(int), hipMemcpyHostToDevice, c->stream));
    c->up_moves = n_moves;
    c->up_max_c = max_c;
    return 0;
}

static int download_results(ig_ctx* c, int n_moves, ig_move_result* results)
{
    const size_t bytes = (size_t)n_moves * sizeof(ig_move_result);
    ig_move_result* stage = (c->h_stage && c->h_stage_bytes >= bytes) ? (ig_move_result*)c->h_stage : nullptr;
    HIPCK(hipMemcpyAsync(stage ? stage : results, c->d_results, bytes, hipMemcpyDeviceToHost, c->stream));
    if (queue_max_readback(c)) return -1;
    HIPCK(hipStreamSynchronize(c->stream));
    if (stage) memcpy(results, stage, bytes);
    HIPCK(hipGetLastError());
    {
        size_t pending = 0; /* timer events are read when the times are asked for (ig_kernel_time_ms), not inside every call */
        for (int i = 0; i < T_COUNT; i++) pending += c->timers[i].ev.size();
        if (pending > 4096) drain_timers(c);
    }
    take_max_readback(c);
    c->full_windows = false;
    for (int i = 0; i < n_moves; i++)
        if (results[i].error) return fail("device-side consistency failure %d at move %d", results[i].error, i);
    return 0;
}

/* one-move path: the lists of the move did not fit the slice pool (ig_move_result.pad = 1: the chooser raised Glob.retry_pool,
 * the apply kernels skipped) -- a larger pool, the flag cleared, and the caller repeats the move.  The batch path has its own way
 * (the decide step stops in front of such a slot: commit loop); until round 4 the one-move path scored such a move WITHOUT the
 * lists that did not fit (found by tools/fuzz_batches.py: nine candidates on contigs that hold a fifth of the contacts each). */
static int retry_with_larger_pool(ig_ctx* c)
{
    if (grow_slice_pool(c)) { /* (synchronises the stream; fails once the pool holds the worst case of a move, or without memory) */
        /* the flag must not outlive the failed call: while it stands every k_apply skips and every k_commit reports pad = 1 -- also
         * for the pending windowed winners of the batch path, which never looks at pad */
        if (hipMemsetAsync(&c->glob->retry_pool, 0, sizeof(int), c->stream) == hipSuccess) (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        return -1;
    }
    HIPCK(hipMemsetAsync(&c->glob->retry_pool, 0, sizeof(int), c->stream));
    c->n_pool_retries++;
    return 0;
}

/* one move per launch sequence until its lists fit the slice pool: attempt() enqueues the move and what reads its outcome back, waits for
 * it and answers 1: it fitted, 0: it did not (a larger pool, again), -1: an error */
template <class Attempt>
static int until_it_fits(ig_ctx* c, Attempt attempt)
{
    for (;;) {
        const int fit = attempt();
        if (fit) return fit < 0 ? -1 : 0;
        if (retry_with_larger_pool(c)) return -1;
    }
}

/* ---- the driver's shared pieces (DESIGN 4.1): what the loops below, ig_batch_commit, ig_step_draw and the runs of ig_host_nuis.inc say once */
/* a launch's FIRST slot was refused (commit_loop: *next_out = -code; the runs: bo[2]) and nothing was committed -- room for it, then the
 * caller scores the same launch again: 1 the slice pool is grown, 2 the exact kernel's grid is made four times larger, 3 a score of exactly
 * 0.0: nothing to do, wait_commit has set exact_next and the next scoring leaves the screening tier out.  `who`: what did not fit. */
static int make_room(ig_ctx* c, int code, const char* who)
{
    if (code == 1) return grow_slice_pool(c);
    if (code == 3) return 0;
    if (c->exact_grid >= c->mb.work_cap) return fail("the exact kernel's work list cannot hold %s", who);
    c->exact_grid = std::min(c->mb.work_cap, c->exact_grid * 4);
    return 0;
}
/* a launch that committed `next` of its w_now slots was cut short by the slice pool, not by a conflict: twice the room for the launches to
 * come (the pool starts at 2 Z entries; small problems with long contigs need more than that for 24 slots).  1: so it was, 0: no, -1: error */
static int pool_cut_short(ig_ctx* c, int next, int w_now)
{
    if (!(next < w_now && c->last_stop == 1 && (size_t)c->mb.pool_cap < slice_pool_max(c))) return 0;
    HIPCK(hipStreamSynchronize(c->stream));
    return alloc_slice_pool(c, std::min(slice_pool_max(c), (size_t)c->mb.pool_cap * 2)) ? -1 : 1;
}
/* The width follows the conflict rate: where few contigs are left (late in an assembly) nearly every move touches a contig an earlier
 * move of the batch modified, and slots scored behind the first conflict are wasted work.  w_ema: moving average of the moves a launch
 * got through (one that got through all of them counts double: the run was at least that long); the next launch is 1.5 x that, at
 * most Wmax.  Results do not depend on the widths. */
static int next_width(const ig_ctx* c, int Wmax) { return std::max(Wmax > 1 ? 2 : 1, std::min(Wmax, (int)(1.5 * c->w_ema + 1.5))); }
static void feed_width(ig_ctx* c, int next, int w_now, int Wmax)
{
    c->w_ema = 0.6 * c->w_ema + 0.4 * (next >= w_now ? std::min(2.0 * w_now, (double)Wmax) : (double)next);
}

/* the moves [0, n_moves) of the uploaded lists: speculative batches of up to Wmax moves (Wmax == 1: one move per launch
 * sequence).  `ready(first, count)` is called before moves [first, first + count) are enqueued: the fused draw + step entry
 * point waits there for its drawing thread and uploads the candidate lists drawn so far. */
template <class Ready>
static int run_moves(ig_ctx* c, int n_moves, int max_c, int Wmax, Ready ready)
{
    if (Wmax == 1) {
        for (int i = 0; i < n_moves; i++) {
            if (ready(i, 1)) return -1;
            /* (one move per launch sequence is the slow way on purpose: the outcome is read per move -- a move whose lists
             * did not fit the slice pool is repeated with a larger one before the next move builds on it) */
            const int rc = until_it_fits(c, [&]() -> int {
                ig_move_result r;
                if (enqueue_move(c, i, max_c, -1, 2)) return -1;
                enqueue_apply(c, i, 0, 0);
                HIPCK(hipMemcpyAsync(&r, c->d_results + i, sizeof r, hipMemcpyDeviceToHost, c->stream));
                HIPCK(hipStreamSynchronize(c->stream));
                return r.pad != 1;
            });
            if (rc) return -1;
        }
        return 0;
    }
    /* speculative batches: score W moves against the same state, commit the conflict-free prefix on the device,
     * finish a winner that needs the exact delta pass with the one-move tail, continue after it */
    if (c->w_ema <= 0.0 || c->w_ema > Wmax) c->w_ema = Wmax;
    int done = 0;
    while (done < n_moves) {
        const int held = ensure_window_slots(c); /* the longest contig may have grown, and fewer slots may fit behind that */
        if (held < 0) return -1;
        Wmax = std::min(Wmax, held);
        const int w_want = next_width(c, Wmax), w_now = std::min(w_want, n_moves - done);
        if (ready(done, w_now) || enqueue_score(c, done, w_now, max_c, -1, 2)) return -1;
        int next = 0;
        if (commit_loop(c, done, w_now, &next)) return -1;
        if (next < 0) { /* the first slot did not fit: more room, the same batch again (nothing was committed) */
            if (make_room(c, -next, "the first move of a batch")) return -1;
            continue;
        }
        const int cut = pool_cut_short(c, next, w_now);
        if (cut < 0) return -1;
        if (!cut && w_now == w_want) feed_width(c, next, w_now, Wmax); /* (a batch cut short by the end of the run says nothing) */
        done += next;
    }
    return 0;
}

/* ---- the window rule (round 5; DESIGN 4.1: commit rules simulated, rule (iii)).  run_moves throws away every slot behind a batch's
 * first conflict -- 10 % of what a batch of 24 scored, 27 % of a batch of 48 -- which is why 24 was the best width although a launch
 * chain has 142 us of fixed cost.  Here the scored slots form a WINDOW over the moves ahead: a slot stays scored from launch to launch
 * while no contig it reads (its focal bin's, its candidates') is written; each launch chain re-scores the slots that went stale --
 * the decide step reports them (decide_body: stale_mask) --, fills the window up with fresh moves, and decides strictly in order up to
 * the first stale slot, exactly as a batch is decided: live scalars, stale insert flags (every slot's candidate 0 is scored with all
 * block-insert slots), zero-score rule, pending windowed winners.  A slot keeps its buffers while the window moves on: position p of
 * the window lives in physical slot (done + p) mod 64 (MoveBuf.rot), a kernel skips the positions in MoveBuf.keep.
 * Invariant: when a chain's decisions start, every slot of the window was scored against a state that differs from the live one
 * only in contigs the slot does not read -- the host drops from `keep` what the previous chain's scan found, everything when the
 * window buffers were re-allocated (longer contigs) or the next scoring is to be exact in every column (zero-score rule).
 * IG_WINDOW=0: the rule of rounds 1 - 4; IG_WINDOW=n: a window of n slots (default 48, at most 64). */
static int g_window = -1;
static int window_width()
{
    if (g_window < 0) {
        const char* e = getenv("IG_WINDOW");
        g_window = e ? atoi(e) : 48;
        g_window = std::min(std::max(g_window, 0), IG_MAX_BATCH);
    }
    return g_window;
}
extern "C" int ig_set_window(int w)
{
    g_window = std::min(std::max(w, 0), IG_MAX_BATCH);
    return 0;
}

/* the ring of physical slots: the largest power of two the per-slot window buffers leave room for (max_batch_width: long contigs late in a
 * human-scale assembly make a slot gigabytes), at most IG_MAX_BATCH; the window is at most the ring */
static int window_ring(ig_ctx* c, int max_c)
{
    int ring = 1;
    while (2 * ring <= std::min(IG_MAX_BATCH, max_batch_width(c, max_c))) ring *= 2;
    return ring;
}

template <class Ready>
static int run_moves_window(ig_ctx* c, int n_moves, int max_c, int Wmax, Ready ready)
{
    int held = ensure_window_slots(c);
    if (held < 0) return -1;
    int ring = 1; /* physical slots in use: a power of two, as many as the buffers hold (plan_call: window_ring at the call's start) */
    while (2 * ring <= std::min(IG_MAX_BATCH, held)) ring *= 2;
    Wmax = std::min(Wmax, ring);
    struct Restore { /* the other entry points index the slots directly */
        ig_ctx* c;
        ~Restore()
        {
            c->mb.rot = 0;
            c->mb.wmask = 0x7fffffff;
            c->mb.keep = 0ull;
            c->mb.ring = 0;
        }
    } restore{c};
    if (c->w_ema <= 0.0 || c->w_ema > Wmax) c->w_ema = Wmax;
    int done = 0;
    int scored_upto = 0;            /* moves [done, scored_upto) have a scored slot -- unless its bit in `stale` says otherwise */
    unsigned long long stale = 0ull; /* bit p: the slot of move done + p has to be scored again */
    while (done < n_moves) {
        const int sN_before = c->mb.sN, sM_before = c->mb.sM;
        if ((held = ensure_window_slots(c)) < 0) return -1; /* the longest contig may have grown: new strides, nothing in the buffers survives */
        /* (the strides, not the pointers: the allocator may hand the freed block out again) */
        const bool regrown = c->mb.sN != sN_before || c->mb.sM != sM_before;
        if (regrown) { /* ... and fewer slots may fit at the new strides: a smaller ring (everything is dropped anyway) */
            while (ring > 1 && ring > held) ring /= 2;
            Wmax = std::min(Wmax, ring);
            if (c->w_ema > Wmax) c->w_ema = Wmax;
        }
        const int w_want = next_width(c, Wmax), w_now = std::min(w_want, n_moves - done);
        if (ready(done, w_now)) return -1;
        if (regrown || c->exact_next) scored_upto = done;
        const int n_have = std::min(std::max(scored_upto - done, 0), w_now);
        unsigned long long keep = (n_have >= 64 ? ~0ull : ((1ull << n_have) - 1ull)) & ~stale;
        /* a launch of ONE slot is not screened (enqueue_score: W > 1), so its decide step does not look for scores of exactly 0.0
         * (zcheck follows own_screened, per launch) -- a kept slot holds the contender-only records of an earlier, screened chain and
         * needs that check: the last move of a call is scored afresh, every column exact (ADVICE r5: the invariant was implicit) */
        if (w_now == 1) keep = 0ull;
        c->mb.rot = done & (ring - 1);
        c->mb.wmask = ring - 1;
        c->mb.keep = keep;
        {
            /* IG_WINDOW_CHECK=1 (tests, fuzzers): every kept slot is validated against the live genome -- the bins of its candidates and
             * their contigs' lengths when a launch keeps it (k_gather: error 11), its window's fragments in their order when its winner is
             * applied (the commit step: error 12) */
            const int s_chk = getenv("IG_WINDOW_CHECK") ? atoi(getenv("IG_WINDOW_CHECK")) : 0; /* (read per launch: a test toggles it) */
            c->mb.ring = 1 | (s_chk ? 4 : 0);
        }
        c->n_window_slots += w_now - __builtin_popcountll(keep);
        if (enqueue_score(c, done, w_now, max_c, -1, 2)) return -1;
        scored_upto = std::max(scored_upto, done + w_now);
        int next = 0;
        if (commit_loop(c, done, w_now, &next)) return -1;
        if (next < 0) { /* the first slot did not fit: more room, the same window again, every slot of it (nothing was committed) */
            if (make_room(c, -next, "the first move of a batch")) return -1;
            scored_upto = done;
            stale = 0ull;
            continue;
        }
        const int cut = pool_cut_short(c, next, w_now);
        if (cut < 0) return -1;
        if (!cut && w_now == w_want) feed_width(c, next, w_now, Wmax);
        /* what the decide step found stale among the positions it did not commit (c->last_stale: position p of THIS window), seen from
         * the next window's front */
        stale = next >= 64 ? 0ull : (c->last_stale >> next);
        /* (the scan covers the positions of THIS window: a slot scored for a wider one, beyond its end, was not looked at -- forgotten) */
        scored_upto = std::min(scored_upto, done + w_now);
        done += next;
    }
    return 0;
}

/* how a call of n_moves is run: *Wmax moves per batch (1: the initial links are not mutually inverse), *Wwin > 1: under the window rule, with
 * a window of that many slots; the move buffers for it */
static int plan_call(ig_ctx* c, int n_moves, int max_c, int* Wmax, int* Wwin)
{
    *Wmax = c->init_links_inverse ? batch_width(c, max_c) : 1;
    const int ring = window_ring(c, max_c);
    *Wwin = (*Wmax > 1 && window_width() > 1) ? std::min(window_width(), ring) : 0;
    c->full_windows = (*Wmax == 1 && n_moves > 1); /* moves enqueued one behind the other: no host round trip to follow the contig lengths */
    return ensure_move_buffers(c, std::max(8, max_c), *Wwin > 1 ? ring : *Wmax);
}

extern "C" int ig_step_batch(ig_ctx* c, int32_t n_moves, const int32_t* frags, const int32_t* cands, int32_t max_c,
                             ig_move_result* results)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (n_moves <= 0) return 0;
    if (max_c < 1 || max_c > IG_MAX_CANDIDATES) return fail("ig_step_batch: max_c out of range");
    if (c->world > 1) return fail("ig_step_batch: this handle scores a contact shard (ig_set_shard %d/%d): use ig_step_begin / all-reduce / ig_step_finish", c->rank, c->world);
    int Wmax, Wwin;
    if (plan_call(c, n_moves, max_c, &Wmax, &Wwin) || upload_moves(c, n_moves, frags, cands, max_c)) return -1;
    auto ready_fn = [](int, int) { return 0; };
    if (Wwin > 1 ? run_moves_window(c, n_moves, max_c, Wwin, ready_fn) : run_moves(c, n_moves, max_c, Wmax, ready_fn)) return -1;
    return download_results(c, n_moves, results);
}

/* n_moves consecutive step_sampler calls INCLUDING their first step, the candidate draw (CL:1403-1408 -> return_neighbours
 * CL:3103-3141): a host thread draws the lists of the moves ahead on the caller's copy of numpy's MT19937 state
 * (ig_draw.cpp) while the launches of the moves in flight run; the lists are uploaded as they appear.  The draws do not
 * depend on the genome, so the result is the same as drawing before each move.  cands_out [n_moves x n_neighbours]
 * receives the lists (sorted, -1 padded). */
extern "C" int ig_step_batch_draw(ig_ctx* c, ig_neighbours* nb, uint32_t* mt_key624, int32_t* mt_pos, int32_t n_moves,
                                  const int32_t* frags, int32_t n_neighbours, int32_t* cands_out, ig_move_result* results)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (n_moves <= 0) return 0;
    if (!nb || !mt_key624 || !mt_pos || !cands_out) return fail("ig_step_batch_draw: NULL argument");
    const int max_c = n_neighbours;
    if (max_c < 1 || max_c > IG_MAX_CANDIDATES) return fail("ig_step_batch_draw: n_neighbours out of range");
    if (c->world > 1) return fail("ig_step_batch_draw: this handle scores a contact shard (ig_set_shard %d/%d)", c->rank, c->world);
    for (int i = 0; i < n_moves; i++)
        if (frags[i] < 0 || frags[i] >= c->N) return fail("fragment %d out of range", frags[i]);
    int Wmax, Wwin;
    if (plan_call(c, n_moves, max_c, &Wmax, &Wwin) || ensure_io(c, n_moves, max_c)) return -1;
    /* the lists go to the device from pinned staging (layout of h_stage: result records, fragments, candidates) */
    int* st_frags = nullptr;
    int* st_cands = nullptr;
    if (c->h_stage) {
        st_frags = (int*)((char*)c->h_stage + (size_t)n_moves * sizeof(ig_move_result));
        st_cands = st_frags + n_moves;
        memcpy(st_frags, frags, (size_t)n_moves * sizeof(int));
    }
    HIPCK(hipMemcpyAsync(c->d_frags, st_frags ? st_frags : frags, (size_t)n_moves * sizeof(int), hipMemcpyHostToDevice, c->stream));
    c->up_moves = n_moves;
    c->up_max_c = max_c;
    std::atomic<int> drawn(0), draw_rc(0);
    /* the lists of the first moves are drawn here (a call of one batch -- the usual benchmark call is 20 moves -- then needs
     * no thread at all: creating and joining one costs as much as drawing 30 lists), the rest on a thread, ahead of the launches */
    const int chunk = 32;
    const int inline_n = std::min(n_moves, std::max(chunk, Wwin)); /* (the first launch chain's whole window: it must not wait for a thread that is still being created) */
    if (ig_neighbours_draw(nb, mt_key624, mt_pos, frags, inline_n, max_c, cands_out)) return fail("candidate draw failed (fragment out of the distributions' range)");
    drawn.store(inline_n, std::memory_order_release);
    std::thread drawer;
    if (n_moves > inline_n)
        drawer = std::thread([&]() {
            for (int i = inline_n; i < n_moves; i += chunk) {
                const int n = std::min(chunk, n_moves - i);
                if (ig_neighbours_draw(nb, mt_key624, mt_pos, frags + i, n, max_c, cands_out + (size_t)i * max_c)) {
                    draw_rc.store(-1, std::memory_order_release);
                    return;
                }
                drawn.store(i + n, std::memory_order_release);
            }
        });
    int uploaded = 0;
    auto ready_fn = [&](int first, int count) -> int {
        int have;
        while ((have = drawn.load(std::memory_order_acquire)) < first + count)
            if (draw_rc.load(std::memory_order_acquire)) return fail("candidate draw failed (fragment out of the distributions' range)");
        if (have > uploaded) { /* everything drawn so far: the later batches find their lists on the device already */
            for (int i = uploaded; i < have; i++) {
                int C = 0;
                while (C < max_c && cands_out[(size_t)i * max_c + C] >= 0) C++;
                if (validate_move(c, frags[i], cands_out + (size_t)i * max_c, C)) return -1;
            }
            const int* src = cands_out + (size_t)uploaded * max_c;
            if (st_cands) {
                memcpy(st_cands + (size_t)uploaded * max_c, src, (size_t)(have - uploaded) * max_c * sizeof(int));
                src = st_cands + (size_t)uploaded * max_c;
            }
            HIPCK(hipMemcpyAsync(c->d_cands + (size_t)uploaded * max_c, src, (size_t)(have - uploaded) * max_c * sizeof(int),
                                 hipMemcpyHostToDevice, c->stream));
            uploaded = have;
        }
        return 0;
    };
    const int rc = Wwin > 1 ? run_moves_window(c, n_moves, max_c, Wwin, ready_fn) : run_moves(c, n_moves, max_c, Wmax, ready_fn);
    if (drawer.joinable()) drawer.join(); /* the generator state the caller puts back is the one after ALL draws, also on an error */
    if (rc) return -1;
    if (draw_rc.load()) return fail("candidate draw failed");
    return download_results(c, n_moves, results);
}

/* ---- the same, one step at a time, for callers that split the slots of a batch over several GPUs ---------- */

extern "C" int ig_batch_upload(ig_ctx* c, int32_t n_moves, const int32_t* frags, const int32_t* cands, int32_t max_c, int32_t max_w)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (n_moves <= 0) return fail("ig_batch_upload: no moves");
    if (max_w < 1 || max_w > promised_width(c, max_c))
        return fail("ig_batch_upload: batch width %d out of 1..%d (ig_batch_max_width)", max_w, promised_width(c, max_c));
    if (c->world > 1) return fail("ig_batch_upload: contact shards (ig_set_shard) and slot splitting are exclusive");
    /* k_commit_batch counts every genome-distance credit exactly once by a rule on mutually inverse initial links -- also for a
     * batch of one move */
    if (!c->init_links_inverse) return fail("ig_batch_upload: the initial prev / next arrays are not mutually inverse: ig_step / ig_step_batch only");
    if (max_c < 1 || max_c > IG_MAX_CANDIDATES) return fail("ig_batch_upload: max_c out of range");
    if (ensure_move_buffers(c, std::max(8, (int)max_c), max_w)) return -1;
    return upload_moves(c, n_moves, frags, cands, max_c);
}

extern "C" int ig_batch_score(ig_ctx* c, int32_t move0, int32_t W, int32_t slot_begin, int32_t slot_end)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (W < 1 || W > c->mb.capW || move0 < 0 || move0 + W > c->up_moves) return fail("ig_batch_score: batch out of range");
    if (slot_begin < 0 || slot_end > W || slot_begin > slot_end) return fail("ig_batch_score: slot range out of range");
    const int held = ensure_window_slots(c); /* the longest contig may have grown */
    if (held < 0) return -1;
    if (W > held) return fail("ig_batch_score: the window buffers hold %d slots at the present contig lengths (ig_batch_max_width)", held);
    if (enqueue_score(c, move0, W, c->up_max_c, -1, 2, slot_begin, slot_end)) return -1;
    HIPCK(hipGetLastError());
    return 0;
}

extern "C" int ig_batch_records(ig_ctx* c, void** records, int64_t* bytes_per_slot)
{
    IG_JOIN(c);
    if (!c->mb.rec) return fail("ig_batch_records: no batch buffers yet (ig_batch_upload first)");
    *records = c->mb.rec;
    *bytes_per_slot = (int64_t)c->mb.rec_stride;
    return 0;
}

extern "C" int ig_batch_commit(ig_ctx* c, int32_t move0, int32_t W, int32_t* n_committed)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (W < 1 || W > c->mb.capW || move0 < 0 || move0 + W > c->up_moves) return fail("ig_batch_commit: batch out of range");
    int next = 0;
    if (commit_loop(c, move0, W, &next)) return -1;
    if (next < 0) { /* the first slot did not fit: more room, the caller scores the batch again */
        if (make_room(c, -next, "the first move of a batch")) return -1;
        next = 0;
    } else if (pool_cut_short(c, next, W) < 0) {
        return -1;
    }
    *n_committed = next;
    return 0;
}

extern "C" int ig_batch_results(ig_ctx* c, int32_t n_moves, ig_move_result* results)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (n_moves < 0 || n_moves > c->up_moves) return fail("ig_batch_results: out of range");
    return download_results(c, n_moves, results);
}

extern "C" int ig_set_batch_width(int w)
{
    g_batch_w = std::min(std::max(w, 1), IG_MAX_BATCH);
    return 0;
}

/* bytes of the move buffers: {per-window arrays (strides sN, sM), slice pool, everything else sized by slots and candidates} */
extern "C" int ig_scratch_bytes(ig_ctx* c, int64_t out3[3])
{
    IG_JOIN(c);
    const MoveBuf& m = c->mb;
    const int64_t C = (int64_t)m.capC * m.capW;
    out3[0] = (int64_t)m.capC * slots_held(c) * ((int64_t)m.sN * 4 * 3 + (int64_t)m.sM * 4 * 2 + (int64_t)m.sM * NSLOT * 8 + (int64_t)NSLOT * NDYN * m.sN * 4);
    out3[1] = m.pool_cap * (m.packed ? 8 : 12);
    out3[2] = C * (int64_t)(SLICE_SEG * 16 + sizeof(CandMeta) + NSLOT * NCODE * sizeof(ColMeta) + (P_STRIDE + Q_STRIDE) * 8 + IG_N_TMP_STRUCT * 8 +
                            NSLOT * 8 + NSLOT * 16 + 16) +
              (int64_t)m.rec_stride * m.capW + (int64_t)m.work_cap * 8 + (int64_t)c->N * 8;
    return 0;
}

extern "C" int ig_batch_stats(ig_ctx* c, int64_t out3[4])
{
    IG_JOIN(c);
    out3[0] = c->n_batches;
    out3[1] = c->n_batch_committed;
    out3[2] = c->n_batch_pending;
    out3[3] = c->n_batch_predicted;
    return 0;
}

/* {contacts in the CSR rows k_slice walked, contacts in the rows a walk per candidate would have read} since the handle was created */
extern "C" int ig_slice_walk_stats(ig_ctx* c, int64_t out2[2])
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    long long h[2] = {0, 0};
    HIPCK(hipMemcpy(h, (const char*)c->glob + offsetof(Glob, slice_walked), sizeof h, hipMemcpyDeviceToHost));
    out2[0] = h[0];
    out2[1] = h[1];
    return 0;
}

/* the one-move entry points: the move's lists -> d_frags[0], d_cands[0 .. C) ... */
static int upload_one_move(ig_ctx* c, const int* frag, const int* cands, int C)
{
    HIPCK(hipMemcpyAsync(c->d_frags, frag, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(c->d_cands, cands, (size_t)C * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return 0;
}
/* ... and the end of a call that applied its move and has synchronised: launch errors, timers, the bound on the longest contig, the record's verdict */
static int finish_one_move(ig_ctx* c, int error)
{
    HIPCK(hipGetLastError());
    drain_timers(c);
    take_max_readback(c);
    if (error) return fail("device-side consistency failure %d", error);
    return 0;
}

extern "C" int ig_step(ig_ctx* c, int32_t frag_a, const int32_t* cands, int32_t C, ig_move_result* out, double* scores)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (c->world > 1) return fail("ig_step: this handle scores a contact shard (ig_set_shard %d/%d): partial sums only -- use ig_step_begin / all-reduce / ig_step_finish", c->rank, c->world);
    if (validate_move(c, frag_a, cands, C)) return -1;
    if (ensure_move_buffers(c, std::max(8, (int)C))) return -1;
    if (ensure_io(c, 1, C)) return -1;
    /* lists, record and scores through the pinned staging block (ensure_io): a copy from / to the caller's pageable memory blocks
     * the host for 10 - 20 us, and this call makes five of them */
    char* stg = (c->h_stage && c->h_stage_bytes >= 8192) ? (char*)c->h_stage : nullptr;
    int* s_in = stg ? (int*)stg : nullptr;
    ig_move_result* s_res = stg ? (ig_move_result*)(stg + 256) : out;
    double* s_sc = stg ? (double*)(stg + 512) : scores;
    if (s_in) {
        s_in[0] = frag_a;
        for (int i = 0; i < C; i++) s_in[1 + i] = cands[i];
    }
    if (upload_one_move(c, s_in ? s_in : &frag_a, s_in ? s_in + 1 : cands, C)) return -1;
    const int rc = until_it_fits(c, [&]() -> int {
        if (enqueue_move(c, 0, C, -1, 2)) return -1;
        if (scores) HIPCK(hipMemcpyAsync(s_sc, c->mb.scores, (size_t)C * IG_N_TMP_STRUCT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        enqueue_apply(c, 0, 0, 0);
        HIPCK(hipMemcpyAsync(s_res, c->d_results, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
        if (queue_max_readback(c)) return -1;
        HIPCK(hipStreamSynchronize(c->stream));
        if (s_res->pad == 1) take_max_readback(c);
        return s_res->pad != 1;
    });
    if (rc) return -1;
    if (stg) {
        *out = *s_res;
        if (scores) memcpy(scores, s_sc, (size_t)C * IG_N_TMP_STRUCT * sizeof(double));
    }
    return finish_one_move(c, out->error);
}

/* ---- one reference-shaped step_sampler call (CL:1401-1465) with less around the move -------------------------------------------------
 * ig_step as the reference's loop calls it (instagraal.py:221-228) spends 225 us per call at cfg3: two uploads and three downloads
 * through the copy engine, a stream synchronisation, numpy's candidate draw and two ctypes calls around 165 us of kernels, 40 of
 * which are the one-move tail (k_scores, k_delta, k_apply, an O(N) k_post, k_commit).  Here: the candidate draw of return_neighbours
 * (CL:3103-3141) inside the call, on numpy's generator state in place; the move's lists read by k_gather from mapped host memory;
 * the move scored as a BATCH OF ONE and decided and applied by the batch path's fused k_decide_commit (16 us: incremental genome
 * distance, nothing O(N)), whose decide wave also writes the C x 24 scores and whose commit waves the record into mapped host
 * memory, where the host polls for them.  scores == NULL (the reference's loop never looks at all_scores, CL:1414-1454): the batch
 * of one is scored in two tiers like a wider one, the exact kernel (60 - 190 us on all 24 x C columns at cfg3) for the contenders only.  A windowed winner that changes the genome
 * is finished by the one-move tail as in every batch (k_commit publishes then); a move whose lists do not fit the slice pool is
 * repeated with a larger one.  Handles without mapped memory, with kernel timers on or whose initial prev / next links are not
 * mutually inverse take ig_step's way.  nb == NULL: the candidates are the caller's (cands[0 .. *n_cands)). */
static bool wait_host_flag(volatile int* flag, int seq, hipStream_t stream);
static int ensure_host_nuis(ig_ctx* c);

extern "C" int ig_step_draw(ig_ctx* c, ig_neighbours* nb, uint32_t* mt_key624, int32_t* mt_pos, int32_t frag_a, int32_t n_neighbours,
                            int32_t* cands, int32_t* n_cands, ig_move_result* out, double* scores)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!cands || !n_cands || !out) return fail("ig_step_draw: NULL argument");
    int list[IG_MAX_CANDIDATES];
    int C = 0;
    /* everything that can refuse the call is looked at BEFORE the draw: the draw advances numpy's MT19937 state in place, and a caller
     * that catches the error and goes on must find the generator where the reference's would be -- untouched (ADVICE r5) */
    if (nb) {
        if (!mt_key624 || !mt_pos) return fail("ig_step_draw: NULL generator state");
        if (n_neighbours < 1 || n_neighbours > IG_MAX_CANDIDATES) return fail("ig_step_draw: n_neighbours out of 1..%d", IG_MAX_CANDIDATES);
        if (frag_a < 0 || frag_a >= c->N) return fail("fragment %d out of range", frag_a);
    } else {
        C = *n_cands;
        if (C < 1 || C > IG_MAX_CANDIDATES) return fail("a move needs 1..%d candidates (got %d)", IG_MAX_CANDIDATES, C);
        for (int i = 0; i < C; i++) list[i] = cands[i];
    }
    if (!c->host_step) c->host_step = (StepHost*)mapped_block(sizeof(StepHost), (void**)&c->host_step_dev, false); /* (none: ig_step's way) */
    if (ensure_host_nuis(c)) return -1;
    const int s_fast = getenv("IG_STEP_DRAW_FAST") ? atoi(getenv("IG_STEP_DRAW_FAST")) : 1; /* 0: ig_step's way (copies, synchronise; read per call: a test toggles it) */
    const bool fast = c->host_step_dev && c->host_nuis_dev && c->host_bo && !c->timing && s_fast && c->init_links_inverse;
    if (fast && c->nuis_in_flight) return fail("ig_step_draw: a nuisance step is in flight (ig_nuis_end): its record travels through the same mapped block");
    if (check_ready(c)) return -1;
    if (c->world > 1) return fail("ig_step_draw: this handle scores a contact shard (ig_set_shard %d/%d): partial sums only -- use ig_step_begin / all-reduce / ig_step_finish", c->rank, c->world);
    /* ... and what can still fail behind the draw (a list that holds the focal bin, no memory for the buffers) puts the state back */
    struct MtUndo {
        uint32_t key[624];
        int32_t pos;
        uint32_t* k;
        int32_t* p;
        bool armed;
        ~MtUndo()
        {
            if (armed) {
                memcpy(k, key, sizeof key);
                *p = pos;
            }
        }
    } undo;
    undo.armed = false;
    if (nb) {
        memcpy(undo.key, mt_key624, sizeof undo.key);
        undo.pos = *mt_pos;
        undo.k = mt_key624;
        undo.p = mt_pos;
        undo.armed = true;
        int32_t row[IG_MAX_CANDIDATES];
        if (ig_neighbours_draw(nb, mt_key624, mt_pos, &frag_a, 1, n_neighbours, row)) return fail("candidate draw failed (fragment out of the distributions' range)");
        for (int i = 0; i < n_neighbours; i++)
            if (row[i] >= 0) list[C++] = row[i];
    }
    if (validate_move(c, frag_a, list, C)) return -1;
    if (nb) {
        for (int i = 0; i < n_neighbours; i++) cands[i] = i < C ? list[i] : -1;
        *n_cands = C;
    }
    if (fast) c->full_windows = false;
    if (ensure_move_buffers(c, std::max(8, (int)C)) || ensure_io(c, 1, C)) return -1;
    undo.armed = false; /* the move is on its way (ig_step: behind its own checks, all passed above, it enqueues the move) */
    if (!fast) return ig_step(c, frag_a, list, C, out, scores);
    StepHost* hs = c->host_step;
    hs->in[0] = frag_a;
    for (int i = 0; i < C; i++) hs->in[1 + i] = list[i];
    c->up_moves = 1;
    c->up_max_c = C;
    struct Restore {
        ig_ctx* c;
        int *f, *cd;
        ~Restore()
        {
            c->d_frags = f;
            c->d_cands = cd;
            c->pub_step = nullptr;
            c->pub_scores = nullptr;
            c->screen_w1 = false;
        }
    } restore{c, c->d_frags, c->d_cands};
    for (;;) {
        if (ensure_window_slots(c) < 0) return -1;
        const int seq = ++c->step_seq;
        c->d_frags = c->host_step_dev->in; /* (k_gather reads the lists from the mapped block: no upload) */
        c->d_cands = c->host_step_dev->in + 1;
        c->pub_step = c->host_step_dev; /* (a windowed winner: the one-move tail's k_commit publishes StepHost.fin) */
        /* the scores wanted: every column through the exact kernel, the decide wave writes them out; not wanted (what the reference's
         * loop does with them: nothing, CL:1414-1454): two-tier scoring as in a wider batch -- every column through the float screen,
         * the exact kernel for the columns that can still win, a score of exactly 0.0 among them the long way (stop code 3) */
        c->pub_scores = scores ? c->host_step_dev->scores : nullptr;
        c->screen_w1 = scores == nullptr;
        const int rc_score = enqueue_score(c, 0, 1, C, -1, 2);
        c->screen_w1 = false;
        c->d_frags = restore.f;
        c->d_cands = restore.cd;
        const long long pend0 = c->n_batch_pending;
        int next = 0;
        const int rc = rc_score ? -1 : commit_loop(c, 0, 1, &next, true);
        c->pub_step = nullptr;
        c->pub_scores = nullptr;
        if (rc) return -1;
        if (next < 0) { /* the move did not fit: more room, again (nothing was committed: run_moves) */
            if (make_room(c, -next, "the move")) return -1;
            if (next == -1) c->n_pool_retries++;
            continue;
        }
        const bool tail = c->n_batch_pending != pend0; /* finished by the one-move tail (k_delta .. k_commit): its record is StepHost.fin */
        if (tail) c->n_step_tail++;
        if (!(tail ? wait_host_flag(&hs->fin_seq, seq, c->stream) : wait_host_flag(&c->host_nuis->res_seq, c->res_seq, c->stream))) {
            HIPCK(hipStreamSynchronize(c->stream));
            return fail("ig_step_draw: the move's kernels ended without its record");
        }
        *out = tail ? hs->fin : c->host_nuis->res;
        c->max_L = std::max(c->max_L, tail ? hs->max_L : c->host_nuis->max_L);
        c->max_SL = std::max(c->max_SL, tail ? hs->max_SL : c->host_nuis->max_SL);
        break;
    }
    HIPCK(hipGetLastError());
    if (scores) memcpy(scores, (const void*)hs->scores, (size_t)C * IG_N_TMP_STRUCT * sizeof(double));
    if (out->error) return fail("device-side consistency failure %d", out->error);
    return 0;
}

extern "C" int ig_score_move(ig_ctx* c, int32_t frag_a, const int32_t* cands, int32_t C, double* scores)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (c->world > 1) return fail("ig_score_move: this handle scores a contact shard (ig_set_shard %d/%d): partial sums only -- use ig_step_begin / all-reduce / ig_step_finish", c->rank, c->world);
    if (validate_move(c, frag_a, cands, C)) return -1;
    if (ensure_move_buffers(c, std::max(8, (int)C))) return -1;
    if (ensure_io(c, 1, C)) return -1;
    if (upload_one_move(c, &frag_a, cands, C)) return -1;
    const int rc = until_it_fits(c, [&]() -> int {
        int retry = 0;
        if (enqueue_move(c, 0, C, -1, 2)) return -1;
        HIPCK(hipMemcpyAsync(scores, c->mb.scores, (size_t)C * IG_N_TMP_STRUCT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(&retry, &c->glob->retry_pool, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return !retry;
    });
    if (rc) return -1;
    HIPCK(hipGetLastError());
    drain_timers(c);
    return 0;
}

extern "C" int ig_apply(ig_ctx* c, int32_t frag_a, int32_t frag_b, int32_t op)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (c->world > 1) return fail("ig_apply: this handle scores a contact shard (ig_set_shard %d/%d): partial sums only -- use ig_step_begin / all-reduce / ig_step_finish", c->rank, c->world);
    if (op < 0 || op >= IG_N_TMP_STRUCT) return fail("ig_apply: op out of range");
    if (validate_move(c, frag_a, &frag_b, 1)) return -1;
    if (ensure_move_buffers(c, 8)) return -1;
    if (ensure_io(c, 1, 1)) return -1;
    if (upload_one_move(c, &frag_a, &frag_b, 1)) return -1;
    ig_move_result r;
    const int rc = until_it_fits(c, [&]() -> int {
        if (enqueue_move(c, 0, 1, op, 2)) return -1;
        enqueue_apply(c, 0, 0, 1);
        HIPCK(hipMemcpyAsync(&r, c->d_results, sizeof r, hipMemcpyDeviceToHost, c->stream));
        if (queue_max_readback(c)) return -1;
        HIPCK(hipStreamSynchronize(c->stream));
        if (r.pad == 1) take_max_readback(c);
        return r.pad != 1;
    });
    return rc ? -1 : finish_one_move(c, r.error);
}

extern "C" int ig_set_shard(ig_ctx* c, int32_t rank, int32_t world)
{
    IG_JOIN(c);
    if (world < 1 || rank < 0 || rank >= world) return fail("ig_set_shard: bad shard %d/%d", rank, world);
    HIPCK(hipStreamSynchronize(c->stream));
    c->rank = rank;
    c->world = world;
    return 0;
}

extern "C" int64_t ig_partials_count(ig_ctx* c) { (void)nuis_join(c); return (int64_t)c->mb.capC * P_STRIDE; }
extern "C" void* ig_partials_device_ptr(ig_ctx* c) { (void)nuis_join(c); return c->mb.part; }

extern "C" int ig_step_begin(ig_ctx* c, int32_t frag_a, const int32_t* cands, int32_t C)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (check_ready(c)) return -1;
    if (validate_move(c, frag_a, cands, C)) return -1;
    if (ensure_move_buffers(c, std::max(8, (int)C))) return -1;
    if (ensure_io(c, 1, C)) return -1;
    if (upload_one_move(c, &frag_a, cands, C)) return -1;
    /* (the partial sums go into a collective next: a rank whose lists did not fit its pool finds out here, on its own) */
    const int rc = until_it_fits(c, [&]() -> int {
        int overflow = 0;
        if (enqueue_move(c, 0, C, -1, 0)) return -1;
        HIPCK(hipMemcpyAsync(&overflow, &c->mb.ctl[0].overflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return !overflow;
    });
    if (rc) return -1;
    HIPCK(hipGetLastError());
    return 0;
}

extern "C" int ig_step_finish(ig_ctx* c, ig_move_result* out, double* scores)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (enqueue_move(c, 0, IG_MAX_CANDIDATES, -1, 1)) return -1;
    if (scores) {
        MoveCtl mc;
        HIPCK(hipMemcpyAsync(&mc, c->mb.ctl, sizeof mc, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        HIPCK(hipMemcpyAsync(scores, c->mb.scores, (size_t)mc.C * IG_N_TMP_STRUCT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    enqueue_apply(c, 0, 0, 0);
    HIPCK(hipMemcpyAsync(out, c->d_results, sizeof(ig_move_result), hipMemcpyDeviceToHost, c->stream));
    if (queue_max_readback(c)) return -1;
    HIPCK(hipStreamSynchronize(c->stream));
    if (finish_one_move(c, out->error)) return -1;
    if (out->pad == 1) { /* (ig_step_begin repeats a move whose lists did not fit: not reachable unless the lists changed in between) */
        HIPCK(hipMemsetAsync(&c->glob->retry_pool, 0, sizeof(int), c->stream));
        return fail("ig_step_finish: the move's lists did not fit the slice pool");
    }
    return 0;
}
