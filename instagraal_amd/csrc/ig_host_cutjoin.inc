/* ig_host_cutjoin.inc -- part of ig_hip.hip (one translation unit; included there in order): cut and join scores, the closed part of
 * the likelihood change of every cut and of every link (ig_kernels_cutjoin.cuh; the rule: instagraal_amd/cut_join.py), and the two
 * host-only entries the rule evaluates its terms with. */

/* the passes ig_debug_cut_join_time reports, in this order */
#define CJ_P_SPAN 0
#define CJ_P_SCAN 1
#define CJ_P_ZERO 2
#define CJ_P_COUNT 3
#define CJ_P_ROWSCAN 4
#define CJ_P_SCATTER 5
#define CJ_P_SORT_SHORT 6
#define CJ_P_SORT_LDS 7
#define CJ_P_SORT_LONG 8
#define CJ_P_REDUCE 9
#define CJ_P_TERMS 10
#define CJ_P_JOIN_ZERO 11
#define CJ_PASSES 12

/* the one free function of the feature: called by ig_destroy, and where the sizes of the genome changed */
static void free_cutjoin_buffers(ig_ctx* c)
{
    CutJoinBuf& b = c->cutjoin;
    hipFree(b.slotl);
    hipFree(b.kof);
    hipFree(b.diff);
    hipFree(b.prof);
    hipFree(b.tot);
    hipFree(b.zcut);
    hipFree(b.srec);
    hipFree(b.brec);
    hipFree(b.vk);
    hipFree(b.vsum);
    hipFree(b.csl);
    hipFree(b.gc);
    hipFree(b.acc);
    hipFree(b.zacc);
    hipFree(b.sc);
    rows_free(b.rows);
    const int form = b.form;
    b = CutJoinBuf{};
    b.form = form;
}

/* the guards of every entry point of the feature: ig_edit_score's */
static int cj_guards(ig_ctx* c, const char* who)
{
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    if (!c->have_state || !c->have_sub) return fail("%s: the sub-fragment table and a state are required", who);
    if (!c->have_params) return fail("%s: set the parameters first", who);
    if (c->nuis_in_flight) return fail("%s: a nuisance step is in flight (ig_nuis_end first)", who);
    if (c->chain_busy) return fail("%s: a chain is in flight (ig_nuis_chain_end first)", who);
    if (c->world != 1) return fail("%s: cut and join scores need all contacts on one handle (this one holds shard %d of %d)", who, c->rank, c->world);
    return 0;
}

/* what the host makes of the state for both reports: the layout of the bins and the numbering of the linear contigs */
struct CjHost {
    std::vector<int> st;            /* the 17 arrays of the state block */
    std::vector<int> slot;          /* [N] first slot of the bin's contig + pos: contigs by ascending id */
    std::vector<int> slotl, kof;    /* [N] the same, -1 on a ring; the number of the bin's contig among the linear ones, -1 on a ring */
    std::vector<int> heads;         /* the first bin of every contig, by ascending contig id */
    std::vector<int> head, tail, nsub, lbp; /* [K] per linear contig */
    int K = 0;
};

/* the buffers sized by N and M (a genome of other sizes, smaller ones included, frees EVERY buffer of the feature -- those sized by the
 * contigs and the pairs too -- and allocates these again), the state on the host, the layout and the linear contigs' sizes on the
 * device (csl, gc: grow-only while N and M stay).  Waits for the stream. */
static int cj_prepare(ig_ctx* c, const char* who, CjHost& h)
{
    CutJoinBuf& b = c->cutjoin;
    const size_t n = (size_t)c->N, m = (size_t)c->M;
    if (b.N != c->N || b.M != c->M) {
        free_cutjoin_buffers(c);
        DALLOC(b.slotl, n);
        DALLOC(b.kof, n);
        DALLOC(b.diff, CJ_ARRAYS * (n + 1));
        DALLOC(b.prof, CJ_ARRAYS * (n + 1));
        DALLOC(b.tot, (size_t)std::max(CJ_ARRAYS * scan_chunks((long long)n + 1), 2 * scan_chunks((long long)m + 2)));
        DALLOC(b.zcut, 2 * n);
        DALLOC(b.srec, m);
        DALLOC(b.brec, 2 * n);
        DALLOC(b.vk, 2 * (m + 2));
        DALLOC(b.vsum, 2 * (m + 2));
        DALLOC(b.sc, 1);
        b.N = c->N;
        b.M = c->M;
    }
    HIPCK(hipStreamSynchronize(c->stream));
    h.st.resize(17 * n);
    HIPCK(hipMemcpy(h.st.data(), c->st_block, 17 * n * sizeof(int), hipMemcpyDeviceToHost));
    const int *pos = &h.st[0], *cid = &h.st[2 * n], *circ = &h.st[4 * n], *next = &h.st[6 * n], *L = &h.st[7 * n], *SL = &h.st[8 * n], *LB = &h.st[9 * n];
    int max_cid = -1;
    for (size_t f = 0; f < n; f++) {
        if (cid[f] < 0) return fail("%s: bin %zu has the contig id %d (inconsistent state)", who, f, cid[f]);
        max_cid = std::max(max_cid, cid[f]);
        if (pos[f] == 0) h.heads.push_back((int)f);
    }
    std::sort(h.heads.begin(), h.heads.end(), [&](int a, int b2) { return cid[a] < cid[b2]; });
    std::vector<int> base((size_t)max_cid + 1, -1), knum((size_t)max_cid + 1, -1);
    long long at = 0;
    for (int f : h.heads) {
        if (base[(size_t)cid[f]] >= 0) return fail("%s: contig %d has two first bins (inconsistent state)", who, cid[f]);
        if (L[f] < 1 || at + L[f] > (long long)n) return fail("%s: the contigs hold more bins than the state (inconsistent state)", who);
        base[(size_t)cid[f]] = (int)at;
        at += L[f];
        if (circ[f] == 0) {
            knum[(size_t)cid[f]] = h.K++;
            h.head.push_back(f);
            h.nsub.push_back(SL[f]);
            h.lbp.push_back(LB[f]);
        }
    }
    if (at != (long long)n) return fail("%s: the contigs hold %lld of %zu bins (inconsistent state)", who, at, n);
    h.tail.assign((size_t)h.K, -1);
    h.slot.resize(n);
    h.slotl.resize(n);
    h.kof.resize(n);
    std::vector<char> seen(n, 0);
    for (size_t f = 0; f < n; f++) {
        const int bs = base[(size_t)cid[f]];
        const long long s = (long long)bs + pos[f];
        if (bs < 0 || pos[f] < 0 || s >= (long long)n || seen[(size_t)s]) return fail("%s: bin %zu has no place of its own in its contig (inconsistent state)", who, f);
        seen[(size_t)s] = 1;
        const int k = circ[f] == 0 ? knum[(size_t)cid[f]] : -1;
        if (circ[f] == 0 && k < 0) return fail("%s: contig %d is linear on bin %zu and a ring on its first bin (inconsistent state)", who, cid[f], f);
        h.slot[f] = (int)s;
        h.slotl[f] = k >= 0 ? (int)s : -1;
        h.kof[f] = k;
        if (k >= 0 && next[f] < 0) h.tail[(size_t)k] = (int)f;
    }
    HIPCK(hipMemcpy(b.slotl, h.slotl.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(b.kof, h.kof.data(), n * sizeof(int), hipMemcpyHostToDevice));
    if (b.cap_K < h.K) {
        hipFree(b.csl);
        hipFree(b.gc);
        b.csl = nullptr;
        b.gc = nullptr;
        b.cap_K = 0;
        const long long cap = (long long)h.K + h.K / 2;
        DALLOC(b.csl, (size_t)cap);
        DALLOC(b.gc, 2 * (size_t)cap);
        b.cap_K = cap;
    }
    if (h.K > 0) HIPCK(hipMemcpy(b.csl, h.nsub.data(), (size_t)h.K * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

/* what eval_q's trans branch makes of the parameters alone (CjTrans, ig_kernels_cutjoin.cuh), with the functions the device uses */
static CjTrans cj_trans_const(const ig_params& p)
{
    const double* T = ig_tab();
    const ig_hot h = ig_hot_make(p, T);
    CjTrans c;
    c.fast = h.fast;
    c.pad = 0;
    c.lg = h.log2_v_inter * IG_LOG2_10_INV;
    c.ex = h.fast ? ig_exp2_core(h.log2_v_inter, T) : 0.0;
    c.vz = (double)p.v_inter * IG_LOG_E_F;
    c.e = (double)p.v_inter;
    c.l10 = ig_log10(c.e, T);
    return c;
}

/* the first rank p >= 1 with (float) p x mean_kb not below d_max, M + 1 where there is none up to M (or the product does not grow
 * with the rank: everything is evaluated then, which is the definition) */
static int cj_pstar(float mean_kb, float d_max, int M)
{
    if (!(mean_kb > 0.0f)) return M + 1;
    int lo = 1, hi = M + 1; /* the answer lies in [lo, hi] */
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((float)mid * mean_kb < d_max) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* the prefix table of the zero-pixel terms beyond p* (enqueued; built only where a contig can reach beyond p*) */
static CjZeroTab cj_enqueue_zero_tab(ig_ctx* c, const Glob& hg)
{
    CutJoinBuf& b = c->cutjoin;
    const int n = c->M + 2;
    CjZeroTab zt;
    zt.pstar = cj_pstar(hg.mean_kb, hg.par[0].d_max, c->M);
    zt.hi = (const long long*)b.vsum;
    zt.lo = (const long long*)b.vsum + n;
    if (zt.pstar <= c->M) {
        hipLaunchKernelGGL(k_cj_vk, dim3((n + CJ_THREADS - 1) / CJ_THREADS), dim3(CJ_THREADS), 0, c->stream, c->glob, n, b.vk, b.vk + n);
        scan64_enqueue(c, b.vk, b.vsum, n, n, 2, b.tot);
    }
    return zt;
}

/* maintained sums + d against the maintained sums, as ig_edit_score's callers form a delta: (nz + z) of the one minus (nz + z) of the other */
static double cj_delta(const Glob& hg, const long long d[5])
{
    const long long h0[5] = {hg.nz_hi, hg.nz_lo, hg.z_hi, hg.z_lo, hg.n_intra};
    long long h1[5];
    for (int k = 0; k < 5; k++) h1[k] = h0[k] + d[k];
    double nz0, z0, nz1, z1;
    likelihood_of_limbs(h0, hg.n_tot_pxl, hg.par[0].v_inter, &nz0, &z0);
    likelihood_of_limbs(h1, hg.n_tot_pxl, hg.par[0].v_inter, &nz1, &z1);
    return (nz1 + z1) - (nz0 + z0);
}

/* the maintained sums and the parameters, as of now */
static int cj_glob(ig_ctx* c, Glob* hg)
{
    flush_pending_sums(c);
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipMemcpy(hg, c->glob, sizeof *hg, hipMemcpyDeviceToHost));
    return 0;
}

static int cut_scores_impl(ig_ctx* c, const char* who, int32_t* valid, int64_t* contacts, int64_t* limbs, double* delta, float* ms)
{
    if (!valid || !contacts || !limbs || !delta) return fail("%s: NULL output", who);
    if (cj_guards(c, who)) return -1;
    LiftTimer timer(c, ms, CJ_PASSES);
    Glob hg;
    if (cj_glob(c, &hg)) return -1;
    CjHost h;
    if (cj_prepare(c, who, h)) return -1;
    CutJoinBuf& b = c->cutjoin;
    const size_t n = (size_t)c->N;
    const long long stride = (long long)n + 1;
    const PzTab pz{c->pz_tab, c->pz_n};
    timer.begin();
    HIPCK(hipMemsetAsync(b.diff, 0, CJ_ARRAYS * (n + 1) * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_cj_sub_records, dim3((c->M + CJ_THREADS - 1) / CJ_THREADS), dim3(CJ_THREADS), 0, c->stream, c->tab, c->sub_tab, b.slotl, c->M, b.srec);
    if (c->Z > 0)
        hipLaunchKernelGGL(k_cut_span, dim3((unsigned)(((long long)c->Z + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0, c->stream, c->crow, c->cc, (long long)c->Z, b.srec, c->glob, c->lgf_tab, pz,
                           cj_trans_const(hg.par[0]), b.diff, stride);
    timer.end(CJ_P_SPAN);
    timer.begin();
    scan64_enqueue(c, b.diff, b.prof, stride, (int)(n + 1), CJ_ARRAYS, b.tot);
    timer.end(CJ_P_SCAN);
    std::vector<long long> prof(CJ_ARRAYS * (n + 1)), zc(2 * n);
    HIPCK(hipMemcpyAsync(prof.data(), b.prof, prof.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    timer.begin();
    const CjZeroTab zt = cj_enqueue_zero_tab(c, hg); /* (its scan takes the chunk totals over from the one above: one stream) */
    if (h.K > 0)
        hipLaunchKernelGGL(k_cj_contig_zero, dim3((unsigned)(((long long)h.K * 64 + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0, c->stream, b.csl, h.K, c->glob,
                           (const float*)c->pz_tab, c->pz_n, zt, b.gc);
    hipLaunchKernelGGL(k_cut_zero, dim3((unsigned)((n * 64 + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0, c->stream, c->st, b.kof, c->N, b.gc, h.K, c->glob,
                       (const float*)c->pz_tab, c->pz_n, zt, b.zcut);
    timer.end(CJ_P_ZERO);
    HIPCK(hipMemcpyAsync(zc.data(), b.zcut, zc.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    /* every contribution closes inside its contig: the sums are zero at every contig's first bin and behind the last one */
    for (int a = 0; a < CJ_ARRAYS; a++) {
        const long long* pr = &prof[(size_t)a * (n + 1)];
        if (pr[n]) return fail("%s: the sums of array %d do not close behind the last contig (%lld; device error)", who, a, pr[n]);
        for (int f : h.heads)
            if (pr[(size_t)h.slot[(size_t)f]]) return fail("%s: the sums of array %d do not close in front of bin %d (%lld; device error)", who, a, f, pr[(size_t)h.slot[(size_t)f]]);
    }
    const int *spos = &h.st[n], *prev = &h.st[5 * n], *SL = &h.st[8 * n];
    for (size_t f = 0; f < n; f++) {
        long long d[5] = {0, 0, 0, 0, 0};
        const bool ok = h.slotl[f] >= 0 && prev[f] >= 0;
        valid[f] = ok;
        contacts[f] = 0;
        if (ok) {
            const size_t s = (size_t)h.slot[f];
            const long long j = spos[f], L = SL[f];
            d[0] = prof[CJ_ARR_HI * (n + 1) + s];
            d[1] = prof[CJ_ARR_LO * (n + 1) + s];
            d[2] = zc[f];
            d[3] = zc[n + f];
            d[4] = -(j * (L - j));
            contacts[f] = prof[CJ_ARR_CNT * (n + 1) + s];
        }
        for (int k = 0; k < 5; k++) limbs[5 * f + k] = d[k];
        delta[f] = ok ? cj_delta(hg, d) : 0.0;
    }
    return 0;
}

extern "C" int ig_cut_scores(ig_ctx* c, int32_t* valid, int64_t* contacts, int64_t* limbs, double* delta)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    return cut_scores_impl(c, "ig_cut_scores", valid, contacts, limbs, delta, nullptr);
}

/* ---- links */

static void cj_drop_result(CutJoinBuf& b)
{
    b.valid = false;
    b.K = b.n_pairs = 0;
    b.h_rowptr.clear();
    b.h_contacts.clear();
    b.h_nz.clear();
    b.h_z.clear();
    b.h_dni.clear();
    b.h_col.clear();
    b.h_head.clear();
    b.h_tail.clear();
    b.h_nsub.clear();
    b.h_lbp.clear();
    b.h_delta.clear();
}

static int join_scores_impl(ig_ctx* c, const char* who, float* ms)
{
    CutJoinBuf& b = c->cutjoin;
    LiftTimer timer(c, ms, CJ_PASSES);
    Glob hg;
    if (cj_glob(c, &hg)) return -1;
    CjHost h;
    if (cj_prepare(c, who, h)) return -1;
    const int K = h.K;
    /* the pairs */
    HIPCK(hipMemsetAsync(b.sc, 0, sizeof(unsigned long long), c->stream));
    auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
        if (c->Z == 0) return;
        const dim3 grid(lift_blocks(c->Z)), block(CJ_THREADS);
        if (!scatter) hipLaunchKernelGGL((k_cj_pairs_emit<false>), grid, block, 0, c->stream, c->crow, c->cc, (long long)c->Z, c->sub_tab, b.kof, slots, ent, n_ent, b.sc);
        else hipLaunchKernelGGL((k_cj_pairs_emit<true>), grid, block, 0, c->stream, c->crow, c->cc, (long long)c->Z, c->sub_tab, b.kof, slots, ent, n_ent, b.sc);
    };
    auto check = [&](long long E) {
        return E < 0 || E > (long long)c->Z || (E > 0 && K < 2) ? fail("%s: %lld entries of %lld contacts (device error)", who, E, (long long)c->Z) : 0;
    };
    /* per entry: the word, the long rows' scratch and their runs' items, a bit, and a pair of its own (column, contacts, ten limbs) */
    const RowsSpec spec = {b.sc, 1, 0, 8 + 8 + 8 + 1 + 4 + 8 + 80, " (fewer pairs of contigs have contacts once the genome is assembled further)", true,
                           {CJ_P_COUNT, CJ_P_ROWSCAN, CJ_P_SCATTER, CJ_P_SORT_SHORT, CJ_P_REDUCE}};
    unsigned long long sc[1];
    long long n_entries = 0, n_pairs = 0;
    if (rows_build(c, who, b.rows, K, spec, sc, check, emit, timer, b.forms, &n_entries, &n_pairs)) return -1;
    if (n_pairs > 0x7fffffffll) return fail("%s: %lld pairs (device error)", who, n_pairs);
    if (b.cap_pairs < n_pairs) {
        hipFree(b.acc);
        hipFree(b.zacc);
        b.acc = b.zacc = nullptr;
        b.cap_pairs = 0;
        const long long cap = n_pairs + n_pairs / 2;
        DALLOC(b.acc, 8 * (size_t)cap);
        DALLOC(b.zacc, 2 * (size_t)cap);
        b.cap_pairs = cap;
    }
    const PzTab pz{c->pz_tab, c->pz_n};
    if (n_pairs > 0) {
        timer.begin();
        HIPCK(hipMemsetAsync(b.acc, 0, 8 * (size_t)n_pairs * sizeof(long long), c->stream));
        const bool lds = b.form < 0 ? n_pairs <= CJ_LDS_PAIRS : b.form == 0;
        const dim3 grid((unsigned)(((long long)c->Z + CJ_THREADS - 1) / CJ_THREADS)), block(CJ_THREADS); /* one contact per thread */
        const CjTrans tc = cj_trans_const(hg.par[0]);
        hipLaunchKernelGGL(k_cj_bin_records, dim3((c->N + CJ_THREADS - 1) / CJ_THREADS), dim3(CJ_THREADS), 0, c->stream, c->st, b.kof, c->N, b.brec);
        if (lds)
            for (long long p0 = 0; p0 < n_pairs; p0 += CJ_LDS_PAIRS) /* (one window by default; a forced form walks them all) */
                hipLaunchKernelGGL((k_cj_join<true>), grid, block, 0, c->stream, c->crow, c->cc, (long long)c->Z, c->sub_tab, b.brec, b.rows.rowptr, b.rows.out_col, (int)n_pairs,
                                   (int)p0, c->glob, c->lgf_tab, pz, tc, b.acc);
        else
            hipLaunchKernelGGL((k_cj_join<false>), grid, block, 0, c->stream, c->crow, c->cc, (long long)c->Z, c->sub_tab, b.brec, b.rows.rowptr, b.rows.out_col, (int)n_pairs, 0,
                               c->glob, c->lgf_tab, pz, tc, b.acc);
        timer.end(CJ_P_TERMS);
        timer.begin();
        const CjZeroTab zt = cj_enqueue_zero_tab(c, hg);
        hipLaunchKernelGGL(k_cj_contig_zero, dim3((unsigned)(((long long)K * 64 + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0, c->stream, b.csl, K, c->glob,
                           (const float*)c->pz_tab, c->pz_n, zt, b.gc);
        hipLaunchKernelGGL(k_cj_join_zero, dim3((unsigned)((n_pairs * 64 + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0, c->stream, b.rows.rowptr, b.rows.out_col, n_pairs,
                           b.csl, K, b.gc, c->glob, (const float*)c->pz_tab, c->pz_n, zt, b.zacc);
        timer.end(CJ_P_JOIN_ZERO);
    }
    /* the result, to the host */
    const size_t np = (size_t)n_pairs;
    b.h_rowptr.assign((size_t)K + 1, 0);
    b.h_col.resize(np);
    b.h_contacts.resize(np);
    b.h_nz.resize(8 * np);
    b.h_z.resize(2 * np);
    HIPCK(hipMemcpyAsync(b.h_rowptr.data(), b.rows.rowptr, ((size_t)K + 1) * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (np) {
        HIPCK(hipMemcpyAsync(b.h_col.data(), b.rows.out_col, np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(b.h_contacts.data(), b.rows.out_cnt, np * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(b.h_nz.data(), b.acc, 8 * np * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(b.h_z.data(), b.zacc, 2 * np * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    if (b.h_rowptr[(size_t)K] != n_pairs) return fail("%s: the rows hold %lld pairs, the build found %lld (device error)", who, b.h_rowptr[(size_t)K], n_pairs);
    b.h_head = h.head;
    b.h_tail = h.tail;
    b.h_nsub = h.nsub;
    b.h_lbp = h.lbp;
    b.h_dni.resize(np);
    b.h_delta.resize(4 * np);
    for (int a = 0; a < K; a++)
        for (long long pr = b.h_rowptr[(size_t)a]; pr < b.h_rowptr[(size_t)a + 1]; pr++) {
            const int bb = b.h_col[(size_t)pr];
            if (bb <= a || bb >= K) return fail("%s: pair %lld of contig %d names contig %d (device error)", who, pr, a, bb);
            b.h_dni[(size_t)pr] = (long long)h.nsub[(size_t)a] * (long long)h.nsub[(size_t)bb];
            for (int q = 0; q < 4; q++) {
                const long long d[5] = {b.h_nz[8 * (size_t)pr + 2 * q], b.h_nz[8 * (size_t)pr + 2 * q + 1], b.h_z[2 * (size_t)pr], b.h_z[2 * (size_t)pr + 1], b.h_dni[(size_t)pr]};
                b.h_delta[4 * (size_t)pr + q] = cj_delta(hg, d);
            }
        }
    b.K = K;
    b.n_pairs = n_pairs;
    return 0;
}

/* the build: whatever happens, what a build needed is gone behind it, and so is the pairs' table on the device (the result is the host's) */
static int join_scores_build(ig_ctx* c, const char* who, float* ms)
{
    CutJoinBuf& b = c->cutjoin;
    cj_drop_result(b);
    if (cj_guards(c, who)) return -1;
    const int rc = join_scores_impl(c, who, ms);
    CutJoinBuf& b2 = c->cutjoin; /* (cj_prepare may have replaced the buffers) */
    rows_free_temp(b2.rows);
    rows_free_result(b2.rows);
    if (rc) {
        cj_drop_result(b2);
        return rc;
    }
    b2.valid = b2.have_forms = true;
    return 0;
}

extern "C" int ig_join_scores_build(ig_ctx* c, int64_t* n_contigs, int64_t* n_pairs)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!n_contigs || !n_pairs) return fail("ig_join_scores_build: NULL output");
    if (join_scores_build(c, "ig_join_scores_build", nullptr)) return -1;
    *n_contigs = c->cutjoin.K;
    *n_pairs = c->cutjoin.n_pairs;
    return 0;
}

extern "C" int ig_join_scores_fetch(ig_ctx* c, int32_t* head_bin, int32_t* tail_bin, int32_t* n_sub, int32_t* length_bp, int64_t* rowptr, int32_t* col, int64_t* contacts,
                                    int64_t* nz, int64_t* z, int64_t* dni, double* delta)
{
    IG_JOIN(c);
    const CutJoinBuf& b = c->cutjoin;
    if (!b.valid) return fail("ig_join_scores_fetch: nothing is built (ig_join_scores_build first)");
    if (!rowptr || (b.K > 0 && (!head_bin || !tail_bin || !n_sub || !length_bp)) || (b.n_pairs > 0 && (!col || !contacts || !nz || !z || !dni || !delta)))
        return fail("ig_join_scores_fetch: NULL output");
    const size_t K = (size_t)b.K, np = (size_t)b.n_pairs;
    memcpy(rowptr, b.h_rowptr.data(), (K + 1) * sizeof(int64_t));
    if (K) {
        memcpy(head_bin, b.h_head.data(), K * sizeof(int32_t));
        memcpy(tail_bin, b.h_tail.data(), K * sizeof(int32_t));
        memcpy(n_sub, b.h_nsub.data(), K * sizeof(int32_t));
        memcpy(length_bp, b.h_lbp.data(), K * sizeof(int32_t));
    }
    if (np) {
        memcpy(col, b.h_col.data(), np * sizeof(int32_t));
        memcpy(contacts, b.h_contacts.data(), np * sizeof(int64_t));
        memcpy(nz, b.h_nz.data(), 8 * np * sizeof(int64_t));
        memcpy(z, b.h_z.data(), 2 * np * sizeof(int64_t));
        memcpy(dni, b.h_dni.data(), np * sizeof(int64_t));
        memcpy(delta, b.h_delta.data(), 4 * np * sizeof(double));
    }
    return 0;
}

extern "C" int ig_join_scores_release(ig_ctx* c)
{
    IG_JOIN(c);
    cj_drop_result(c->cutjoin);
    return 0;
}

extern "C" int ig_debug_cut_join_form(ig_ctx* c, int32_t form)
{
    IG_JOIN(c);
    if (form < -1 || form > 1) return fail("ig_debug_cut_join_form: -1 (by the number of pairs), 0 (LDS) or 1 (atomics per run), got %d", form);
    c->cutjoin.form = form;
    return 0;
}

extern "C" int ig_debug_join_scores_forms(ig_ctx* c, int64_t out8[8])
{
    IG_JOIN(c);
    if (!out8) return fail("ig_debug_join_scores_forms: NULL output");
    if (!c->cutjoin.have_forms) return fail("ig_debug_join_scores_forms: nothing was built (ig_join_scores_build first)");
    for (int k = 0; k < 8; k++) out8[k] = c->cutjoin.forms[k];
    return 0;
}

extern "C" int ig_debug_cut_join_time(ig_ctx* c, int32_t what, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_cut_join_time";
    if (n < 1 || !ms_n) return fail("%s: bad arguments", who);
    if (what != 0 && what != 1) return fail("%s: what is 0 (cuts) or 1 (joins), got %d", who, what);
    std::vector<long long> all;
    if (what == 0) {
        const size_t N = (size_t)c->N;
        std::vector<int32_t> valid(N + 1);
        std::vector<int64_t> contacts(N + 1), limbs(5 * N + 1);
        std::vector<double> delta(N + 1);
        for (int r = 0; r < n; r++)
            if (cut_scores_impl(c, who, valid.data(), contacts.data(), limbs.data(), delta.data(), ms_n + (size_t)r * CJ_PASSES)) return -1;
        all.assign(valid.begin(), valid.end() - 1);
        all.insert(all.end(), contacts.begin(), contacts.end() - 1);
        all.insert(all.end(), limbs.begin(), limbs.end() - 1);
    } else {
        for (int r = 0; r < n; r++)
            if (join_scores_build(c, who, ms_n + (size_t)r * CJ_PASSES)) return -1;
        const CutJoinBuf& b = c->cutjoin;
        all = b.h_rowptr;
        all.insert(all.end(), b.h_col.begin(), b.h_col.end());
        all.insert(all.end(), b.h_contacts.begin(), b.h_contacts.end());
        all.insert(all.end(), b.h_nz.begin(), b.h_nz.end());
        all.insert(all.end(), b.h_z.begin(), b.h_z.end());
        all.insert(all.end(), b.h_dni.begin(), b.h_dni.end());
    }
    if (checksum) *checksum = (long long)weighted_checksum(all.data(), all.size()); /* every form of a pass agrees on it */
    return 0;
}

/* ---- the host-only entries: no context, no GPU */

/* the 15 float-factorial constants of log10(ob!) (KA:111-124), as ig_create builds them */
static void cj_lgf_small(double small[15])
{
    for (int k = 0; k < 15; k++) {
        float r = 1;
        if (k < 10) {
            for (int q = 1; q <= k; q++) r = r * q;
        } else {
            r = ig_powf((float)k, (float)k, ig_tab()) * ig_expf(-(float)k, ig_tab()) * __builtin_sqrtf((float)(2 * 3.14159265358979323846 * (float)k));
        }
        small[k] = ig_log10((double)r, ig_tab());
    }
}

/* eval_q's ring-free branch (ig_model.cuh) on the host from include/ig_detmath.h, hot path selection included: contact k has the
 * separation s[k] (kb), the rank distance d[k], the count count[k]; trans[k] != 0: a trans pair */
extern "C" int ig_contact_terms_host(const float params[8], float mean_kb, const float* s, const int32_t* d, const int32_t* trans, const int32_t* count, int64_t n,
                                     int64_t* q)
{
    if (!params || n < 0 || (n > 0 && (!s || !d || !trans || !count || !q))) return fail("ig_contact_terms_host: bad arguments");
    ig_params p;
    memcpy(&p, params, sizeof(p)); /* (eight floats in the order of ig_params) */
    const double* T = ig_tab();
    const ig_hot h = ig_hot_make(p, T);
    double small[15];
    cj_lgf_small(small);
    for (int64_t k = 0; k < n; k++) {
        const int ob = count[k];
        const double lgf = ob <= 0 ? 0.0 : ig_lgfact(ob, small, T); /* lgfact_dev: the table's entries and lgfact_big are this */
        float ex, ex_z;
        double t;
        if (!trans[k]) {
            const float s_z = (float)d[k] * mean_kb; /* pz_lookup: the table holds pz_direct's values */
            ex_z = (s_z < p.d_max) ? ig_rippe(s_z, p, T) : p.v_inter;
            if (h.fast && ob > 0) {
                q[k] = ig_quantize(ig_term_hot(s[k], 0, ob, lgf, ex_z, &h, T));
                continue;
            }
            ex = ig_rippe(s[k], p, T);
        } else {
            ex = p.v_inter;
            ex_z = p.v_inter;
            if (h.fast && ob > 0) {
                q[k] = ig_quantize(ig_term_hot(0.0f, 1, ob, lgf, ex_z, &h, T));
                continue;
            }
        }
        t = ig_pixel_term(ex, ex_z, ob, lgf, T);
        q[k] = ig_quantize(t);
    }
    return 0;
}

/* zero_q of a linear contig (s_tot == 0) on the host: the sub-fragment of rank pos[k] in a contig of len[k] */
extern "C" int ig_zero_terms_host(const float params[8], float mean_kb, const int32_t* pos, const int32_t* len, int64_t n, int64_t* q)
{
    if (!params || n < 0 || (n > 0 && (!pos || !len || !q))) return fail("ig_zero_terms_host: bad arguments");
    ig_params p;
    memcpy(&p, params, sizeof(p));
    for (int64_t k = 0; k < n; k++) {
        const float s = (float)pos[k] * mean_kb;
        const double ve = (s < p.d_max) ? (double)ig_rippe(s, p, ig_tab()) : (double)p.v_inter;
        q[k] = ig_quantize(0.0 - (ve * (double)(len[k] - pos[k])));
    }
    return 0;
}

/* tests: eval_q on the device for the inputs of ig_contact_terms_host (s >= 0, 0 <= d < 2^28), under parameter set 0 and its P_z table */
extern "C" int ig_debug_contact_terms(ig_ctx* c, const float* s, const int32_t* d, const int32_t* trans, const int32_t* count, int64_t n, int64_t* q)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->have_params) return fail("ig_debug_contact_terms: set the parameters first");
    if (n < 0 || (n > 0 && (!s || !d || !trans || !count || !q))) return fail("ig_debug_contact_terms: bad arguments");
    if (n == 0) return 0;
    float* ds = nullptr;
    int *dd = nullptr, *dt = nullptr, *dc = nullptr;
    long long* dq = nullptr;
    int rc = 0;
    if (dalloc(&ds, (size_t)n, "s") || dalloc(&dd, (size_t)n, "d") || dalloc(&dt, (size_t)n, "trans") || dalloc(&dc, (size_t)n, "count") || dalloc(&dq, (size_t)n, "q")) rc = -1;
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpy(ds, s, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dd, d, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dt, trans, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dc, count, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_debug_contact_terms, dim3((unsigned)((n + CJ_THREADS - 1) / CJ_THREADS)), dim3(CJ_THREADS), 0, c->stream, ds, dd, dt, dc, (long long)n, c->glob,
                               c->lgf_tab, PzTab{c->pz_tab, c->pz_n}, dq);
            e = hipStreamSynchronize(c->stream);
        }
        if (e == hipSuccess) e = hipMemcpy(q, dq, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail("ig_debug_contact_terms: %s", hipGetErrorString(e));
    }
    hipFree(ds);
    hipFree(dd);
    hipFree(dt);
    hipFree(dc);
    hipFree(dq);
    return rc;
}
