/* ig_host_edit.inc -- part of ig_hip.hip (one translation unit; included there in order): segment edits, scored exactly and applied
 * (ig_kernels_edit.cuh; the rule: instagraal_amd/rearrange.py). */

/* the passes ig_debug_edit_time reports, in this order */
#define EDIT_P_PLAN 0
#define EDIT_P_STATE 1
#define EDIT_P_TABLES 2
#define EDIT_P_DELTA 3
#define EDIT_P_ZERO 4
#define EDIT_P_WHOLE 5
#define EDIT_PASSES 6

/* the one free function of the feature: called by ig_destroy, and where the sizes of the genome changed */
static void free_edit_buffers(ig_ctx* c)
{
    EditBuf& b = c->edit;
    hipFree(b.edits);
    hipFree(b.plan);
    hipFree(b.dyn);
    hipFree(b.dist);
    hipFree(b.stot);
    hipFree(b.len);
    hipFree(b.cp);
    hipFree(b.mask);
    hipFree(b.acc);
    b = EditBuf{};
}

/* device bytes one edit of a chunk needs: its scratch state and its scratch tables */
static unsigned long long edit_bytes_per_edit(int N, int M) { return (unsigned long long)NDYN * (unsigned long long)N * 4ull + 20ull * (unsigned long long)M + 5ull * 4ull + sizeof(EditPlan); }

/* the largest chunk (<= EDIT_CHUNK, <= n_edits) whose buffers fit `free_b` bytes next to `fixed` bytes; 0: not even one edit fits */
static int edit_chunk_for(unsigned long long free_b, unsigned long long fixed, unsigned long long per_edit, int n_edits)
{
    if (free_b < fixed) return 0;
    const unsigned long long fit = (free_b - fixed) / per_edit;
    return (int)std::min<unsigned long long>(fit, (unsigned long long)std::min(n_edits, EDIT_CHUNK));
}

/* the buffers for chunks of up to `want` edits (grow-only; kept from call to call) -> *chunk: the edits a chunk may hold */
static int edit_reserve(ig_ctx* c, const char* who, int want, int next_cid, int* chunk)
{
    EditBuf& b = c->edit;
    if (b.N != c->N || b.M != c->M) free_edit_buffers(c);
    const size_t mask_need = (size_t)next_cid + 1;
    if (b.mask_cap < mask_need) {
        hipFree(b.mask);
        b.mask = nullptr;
        b.mask_cap = 0;
        DALLOC(b.mask, mask_need + mask_need / 2);
        b.mask_cap = mask_need + mask_need / 2;
    }
    if (!b.acc) DALLOC(b.acc, (size_t)EDIT_CHUNK * EDIT_ACC);
    want = std::max(1, std::min(want, EDIT_CHUNK));
    if (b.cap < want) {
        const unsigned long long per = edit_bytes_per_edit(c->N, c->M);
        size_t free_b = ~(size_t)0, total_b = 0;
        if (&hipMemGetInfo != nullptr) HIPCK(hipMemGetInfo(&free_b, &total_b));
        /* what the handle holds already goes back first: the new set replaces it */
        const unsigned long long held = (unsigned long long)b.cap * per;
        const int cap = edit_chunk_for((unsigned long long)free_b + held, 1ull << 20, per, want);
        if (cap < 1) return fail("%s: one edit needs %llu bytes of device memory for its scratch state and tables, %zu are free", who, per + (1ull << 20), free_b);
        hipFree(b.edits);
        hipFree(b.plan);
        hipFree(b.dyn);
        hipFree(b.dist);
        hipFree(b.stot);
        hipFree(b.len);
        hipFree(b.cp);
        b.edits = nullptr;
        b.plan = nullptr;
        b.dyn = nullptr;
        b.dist = b.stot = nullptr;
        b.len = nullptr;
        b.cp = nullptr;
        b.cap = 0;
        DALLOC(b.edits, (size_t)cap * 5);
        DALLOC(b.plan, (size_t)cap);
        DALLOC(b.dyn, (size_t)cap * NDYN * (size_t)c->N);
        DALLOC(b.dist, (size_t)cap * (size_t)c->M);
        DALLOC(b.stot, (size_t)cap * (size_t)c->M);
        DALLOC(b.len, (size_t)cap * (size_t)c->M);
        DALLOC(b.cp, (size_t)cap * (size_t)c->M);
        b.cap = cap;
        b.N = c->N;
        b.M = c->M;
    }
    *chunk = std::min(b.cap, want);
    return 0;
}

/* the guards of every entry point of the feature: genome_view's, and one handle with all contacts */
static int edit_guards(ig_ctx* c, const char* who)
{
    if (!c->have_contacts) return fail("%s: upload the contacts first", who);
    if (!c->have_state || !c->have_sub) return fail("%s: the sub-fragment table and a state are required", who);
    if (!c->have_params) return fail("%s: set the parameters first", who);
    if (c->nuis_in_flight) return fail("%s: a nuisance step is in flight (ig_nuis_end first)", who);
    if (c->chain_busy) return fail("%s: a chain is in flight (ig_nuis_chain_end first)", who);
    if (c->world != 1) return fail("%s: segment edits need all contacts on one handle (this one holds shard %d of %d)", who, c->rank, c->world);
    return 0;
}

/* the scratch state of edit e as a State: its dynamic arrays, the live constant ones */
static State edit_state_of(ig_ctx* c, int e)
{
    State s = c->st;
    int** sp = (int**)&s;
    for (int k = 0; k < NDYN; k++) sp[k] = c->edit.dyn + ((size_t)e * NDYN + (size_t)k) * (size_t)c->N;
    return s;
}

/* plan, scratch states and scratch tables of `n` edits (<= the reserved chunk), enqueued */
static int edit_enqueue_states(ig_ctx* c, const int32_t* edits, int n, LiftTimer& timer)
{
    EditBuf& b = c->edit;
    const int N = c->N, M = c->M;
    HIPCK(hipMemcpyAsync(b.edits, edits, (size_t)n * 5 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemsetAsync(b.mask, 0, b.mask_cap * sizeof(unsigned long long), c->stream));
    timer.begin();
    hipLaunchKernelGGL(k_edit_plan, dim3(1), dim3(EDIT_CHUNK), 0, c->stream, c->st, c->glob, b.edits, n, N, b.plan, b.mask, (int)std::min<size_t>(b.mask_cap, 0x7fffffff));
    timer.end(EDIT_P_PLAN);
    timer.begin();
    hipLaunchKernelGGL(k_edit_state, dim3((N + EDIT_THREADS - 1) / EDIT_THREADS, n), dim3(EDIT_THREADS), 0, c->stream, c->st, b.plan, N, b.dyn);
    timer.end(EDIT_P_STATE);
    timer.begin();
    const EditTabs et{b.dist, b.stot, b.len, b.cp};
    for (int e = 0; e < n; e++)
        hipLaunchKernelGGL(k_fill_tables, dim3((M + 255) / 256), dim3(256), 0, c->stream, edit_state_of(c, e), c->sub_tab, edit_tables(et, e, M), M);
    timer.end(EDIT_P_TABLES);
    return 0;
}

/* the call: chunks of the list through the plan, the states, the tables and the form's sums */
static int edit_score_impl(ig_ctx* c, const char* who, int n_edits, const int32_t* edits, int form, int32_t* status, int64_t* limbs, double* nz, double* z, float* ms)
{
    if (n_edits < 0) return fail("%s: list of %d edits", who, n_edits);
    if (n_edits > 0 && (!edits || !status || !limbs || !nz || !z)) return fail("%s: NULL argument", who);
    if (form != 0 && form != 1) return fail("%s: form is 0 (delta) or 1 (whole), got %d", who, form);
    if (edit_guards(c, who)) return -1;
    LiftTimer timer(c, ms, EDIT_PASSES);
    if (n_edits == 0) return 0;
    flush_pending_sums(c);
    HIPCK(hipStreamSynchronize(c->stream));
    Glob hg;
    HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
    int chunk = 0;
    if (edit_reserve(c, who, n_edits, hg.next_cid, &chunk)) return -1;
    EditBuf& b = c->edit;
    const int M = c->M;
    const EditTabs et{b.dist, b.stot, b.len, b.cp};
    const PzTab pz{c->pz_tab, c->pz_n};
    std::vector<EditPlan> plans((size_t)chunk);
    std::vector<long long> acc((size_t)chunk * EDIT_ACC);
    for (int e0 = 0; e0 < n_edits; e0 += chunk) {
        const int n = std::min(chunk, n_edits - e0);
        if (edit_enqueue_states(c, edits + (size_t)e0 * 5, n, timer)) return -1;
        HIPCK(hipMemcpyAsync(plans.data(), b.plan, (size_t)n * sizeof(EditPlan), hipMemcpyDeviceToHost, c->stream));
        if (form == 0) {
            HIPCK(hipMemsetAsync(b.acc, 0, (size_t)EDIT_CHUNK * EDIT_ACC * sizeof(long long), c->stream));
            timer.begin();
            if (c->Z > 0)
                hipLaunchKernelGGL(k_edit_delta, dim3(lift_blocks(c->Z)), dim3(EDIT_THREADS), 0, c->stream, c->crow, c->cc, (long long)c->Z, c->tab, et, M, b.mask,
                                   (int)std::min<size_t>(b.mask_cap, 0x7fffffff), c->glob, c->lgf_tab, pz, b.acc);
            timer.end(EDIT_P_DELTA);
            timer.begin();
            hipLaunchKernelGGL(k_edit_zero_delta, dim3(std::min((M + EDIT_THREADS - 1) / EDIT_THREADS, 1024)), dim3(EDIT_THREADS), 0, c->stream, c->tab, et, M, b.mask,
                               (int)std::min<size_t>(b.mask_cap, 0x7fffffff), c->glob, (const float*)c->pz_tab, c->pz_n, b.acc);
            timer.end(EDIT_P_ZERO);
            HIPCK(hipMemcpyAsync(acc.data(), b.acc, (size_t)n * EDIT_ACC * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
            HIPCK(hipStreamSynchronize(c->stream));
            for (int e = 0; e < n; e++) {
                long long h[5] = {hg.nz_hi + acc[(size_t)e * EDIT_ACC], hg.nz_lo + acc[(size_t)e * EDIT_ACC + 1], hg.z_hi + acc[(size_t)e * EDIT_ACC + 2],
                                  hg.z_lo + acc[(size_t)e * EDIT_ACC + 3], hg.n_intra + acc[(size_t)e * EDIT_ACC + 4]};
                ig_acc_normalize((int64_t*)&h[0], (int64_t*)&h[1]);
                ig_acc_normalize((int64_t*)&h[2], (int64_t*)&h[3]);
                for (int k = 0; k < 5; k++) limbs[(size_t)(e0 + e) * 5 + k] = h[k];
            }
        } else {
            timer.begin();
            for (int e = 0; e < n; e++) { /* the definition: the from-scratch passes of ig_full_likelihood on the tables of edit e */
                long long* scratch = c->scratch8;
                const Tables t = edit_tables(et, e, M);
                HIPCK(hipMemsetAsync(scratch, 0, 8 * sizeof(long long), c->stream));
                if (!launch_full_nz(c, t, 0, scratch, pz, nullptr, scratch + 2))
                    hipLaunchKernelGGL(k_full_zero, dim3(128), dim3(256), 0, c->stream, t, c->glob, 0, M, scratch + 2);
                long long h[8];
                HIPCK(hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, c->stream));
                HIPCK(hipStreamSynchronize(c->stream));
                ig_acc_normalize((int64_t*)&h[0], (int64_t*)&h[1]);
                ig_acc_normalize((int64_t*)&h[2], (int64_t*)&h[3]);
                for (int k = 0; k < 5; k++) limbs[(size_t)(e0 + e) * 5 + k] = h[k];
            }
            timer.end(EDIT_P_WHOLE);
            HIPCK(hipStreamSynchronize(c->stream));
        }
        for (int e = 0; e < n; e++) {
            status[e0 + e] = plans[(size_t)e].status;
            long long h[5];
            for (int k = 0; k < 5; k++) h[k] = limbs[(size_t)(e0 + e) * 5 + k];
            likelihood_of_limbs(h, hg.n_tot_pxl, hg.par[0].v_inter, &nz[e0 + e], &z[e0 + e]); /* (ig_host_upload.inc: as ig_full_likelihood forms them) */
        }
    }
    return 0;
}

extern "C" int ig_edit_score(ig_ctx* c, int32_t n_edits, const int32_t* edits, int32_t form, int32_t* status, int64_t* limbs, double* nz, double* z)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    return edit_score_impl(c, "ig_edit_score", n_edits, edits, form, status, limbs, nz, z, nullptr);
}

/* the scratch state of one edit, enqueued and waited for -> its status */
static int edit_one_state(ig_ctx* c, const char* who, const int32_t edit[5], int* status, int* anchor_new)
{
    if (!edit || !status) return fail("%s: NULL argument", who);
    if (edit_guards(c, who)) return -1;
    flush_pending_sums(c);
    HIPCK(hipStreamSynchronize(c->stream));
    int next_cid = 0;
    HIPCK(hipMemcpy(&next_cid, &c->glob->next_cid, sizeof(int), hipMemcpyDeviceToHost));
    int chunk = 0;
    if (edit_reserve(c, who, 1, next_cid, &chunk)) return -1;
    LiftTimer timer(c, nullptr, EDIT_PASSES);
    if (edit_enqueue_states(c, edit, 1, timer)) return -1;
    EditPlan p;
    HIPCK(hipMemcpyAsync(&p, c->edit.plan, sizeof p, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    *status = p.status;
    if (anchor_new) *anchor_new = edit[2] == EDIT_NEW_CONTIG;
    return 0;
}

extern "C" int ig_edit_state(ig_ctx* c, const int32_t edit[5], int32_t* soa, int32_t* status)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_edit_state";
    if (!soa || !status) return fail("%s: NULL argument", who);
    int st = 0;
    if (edit_one_state(c, who, edit, &st, nullptr)) return -1;
    *status = st;
    const size_t n = (size_t)c->N;
    std::vector<int> dyn(NDYN * n), con(6 * n);
    HIPCK(hipMemcpy(dyn.data(), c->edit.dyn, NDYN * n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(con.data(), c->st_block + NDYN * n, 6 * n * sizeof(int), hipMemcpyDeviceToHost));
    static const int dyn_src[NDYN] = {0, 1, 2, 3, 6, 8, 9, 10, 11, 12, 13}; /* as ig_download_state, with the internal contig ids */
    for (int k = 0; k < NDYN; k++) memcpy(soa + dyn_src[k] * n, &dyn[k * n], n * sizeof(int));
    memcpy(soa + 4 * n, &con[0], n * sizeof(int));      /* len_bp */
    memcpy(soa + 5 * n, &con[n], n * sizeof(int));      /* sub_len */
    memcpy(soa + 14 * n, &con[3 * n], n * sizeof(int)); /* rep */
    memcpy(soa + 15 * n, &con[4 * n], n * sizeof(int)); /* activ */
    memcpy(soa + 16 * n, &con[5 * n], n * sizeof(int)); /* id_d */
    for (size_t f = 0; f < n; f++) soa[7 * n + f] = (int)f;
    return 0;
}

extern "C" int ig_edit_apply(ig_ctx* c, const int32_t edit[5], int32_t* status, int64_t* limbs5)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_edit_apply";
    if (!status) return fail("%s: NULL argument", who);
    int st = 0, is_new = 0;
    if (edit_one_state(c, who, edit, &st, &is_new)) return -1;
    *status = st;
    if (st == 0) { /* (a refused edit leaves everything as it was) */
        c->nuis_spec = c->spec_valid = false; /* moves scored ahead were scored on the genome that goes away now */
        hipLaunchKernelGGL(k_edit_commit, dim3((c->N + EDIT_THREADS - 1) / EDIT_THREADS), dim3(EDIT_THREADS), 0, c->stream, c->st, c->edit.dyn, c->N, c->glob, is_new);
        if (launch_recompute(c)) return -1;
    }
    if (limbs5) {
        Glob hg;
        HIPCK(hipMemcpy(&hg, c->glob, sizeof hg, hipMemcpyDeviceToHost));
        limbs5[0] = hg.nz_hi;
        limbs5[1] = hg.nz_lo;
        limbs5[2] = hg.z_hi;
        limbs5[3] = hg.z_lo;
        limbs5[4] = hg.n_intra;
    }
    return 0;
}

extern "C" int ig_debug_edit_time(ig_ctx* c, int32_t n_edits, const int32_t* edits, int32_t form, int32_t n, float* ms_n, int64_t* checksum)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_debug_edit_time";
    if (n < 1 || !ms_n) return fail("%s: bad arguments", who);
    if (n_edits < 0) return fail("%s: list of %d edits", who, n_edits);
    const size_t ne = (size_t)n_edits;
    std::vector<int32_t> status(ne + 1);
    std::vector<int64_t> limbs(5 * ne + 1);
    std::vector<double> nz(ne + 1), z(ne + 1);
    for (int r = 0; r < n; r++)
        if (edit_score_impl(c, who, n_edits, edits, form, status.data(), limbs.data(), nz.data(), z.data(), ms_n + (size_t)r * EDIT_PASSES)) return -1;
    if (checksum) { /* of the last result: the statuses, then the limbs, each word weighted by its place: the two forms agree on it */
        std::vector<long long> all(status.begin(), status.end() - 1);
        all.insert(all.end(), limbs.begin(), limbs.end() - 1);
        *checksum = (long long)weighted_checksum(all.data(), all.size());
    }
    return 0;
}
