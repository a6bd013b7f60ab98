/* ig_kernels_edit.cuh -- segment edits (the rule: instagraal_amd/rearrange.py): a run of bins of one linear contig taken out,
 * optionally reversed, and put back, made a contig of its own or inserted next to an anchor bin.  k_edit_plan: the status of every
 * edit and the few boundary values its closed forms need; k_edit_state: the 11 dynamic arrays of every bin under every edit, by closed
 * form from the plan (no scan, no sort); the coordinate tables of every edited state come from k_fill_tables.  The exact sums of an
 * edited genome: the from-scratch passes on its tables (the whole form), or the maintained sums plus k_edit_delta and
 * k_edit_zero_delta (the delta form): ONE pass over the contacts / the sub-fragments for a chunk of up to EDIT_CHUNK edits, which
 * evaluates eval_q / zero_q only where a contig an edit touches is involved. */
#pragma once

#define EDIT_CHUNK 64 /* edits per chunk: one bit each in the masks of the contigs */
#define EDIT_THREADS 256
#define EDIT_IN_PLACE (-2)
#define EDIT_NEW_CONTIG (-1)
#define EDIT_ACC 5 /* per edit: nz hi, nz lo, z hi, z lo, intra pairs (differences against the current genome) */

struct EditPlan {
    int status;
    int first, last;        /* the segment's end bins in the CURRENT order */
    int cs, cd;             /* the segment's contig, the contig it goes to (a NEW_CONTIG: the new id) */
    int a, b, n;            /* ranks of first and last, bins in the segment */
    int flip;
    int sp_a, sp_end;       /* sub_pos at the segment's start and behind its end */
    int bp_a, bp_end;       /* start_bp likewise */
    int r, ins_sub, ins_bp; /* where the segment goes, in the coordinates of the destination WITHOUT the segment */
    int lnb, rnb;           /* the bins in front of and behind the segment at its new place, -1: none */
    int cut_prev, cut_next; /* the bins in front of and behind the segment at its old place */
    int rem_L, rem_SL, rem_LB; /* totals of the remainder */
    int dst_L, dst_SL, dst_LB; /* totals of the destination with the segment */
    int same;               /* the destination is the remainder (IN_PLACE, or an anchor in the segment's own contig) */
    int pad;
};

/* one thread per edit of the chunk; mask[cid] |= 1 << e for the contigs a valid edit touches (cleared by the host) */
__global__ void k_edit_plan(State st, const Glob* g, const int* __restrict__ edits, int n_edits, int N, EditPlan* __restrict__ plan,
                            unsigned long long* __restrict__ mask, int mask_n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edits) return;
    const int fb = edits[5 * e], lb = edits[5 * e + 1], anchor = edits[5 * e + 2], side = edits[5 * e + 3], flip = edits[5 * e + 4];
    EditPlan p;
    memset(&p, 0, sizeof p);
    p.first = fb;
    p.last = lb;
    p.flip = flip;
    int status = 0;
    if (fb < 0 || fb >= N || lb < 0 || lb >= N || anchor >= N) status = 1;
    else if (st.cid[fb] != st.cid[lb] || st.pos[fb] > st.pos[lb]) status = 2;
    else if (st.circ[fb] != 0 || (anchor >= 0 && st.circ[anchor] != 0)) status = 3;
    else if (anchor >= 0 && st.cid[anchor] == st.cid[fb] && st.pos[anchor] >= st.pos[fb] && st.pos[anchor] <= st.pos[lb]) status = 4;
    else if (anchor < EDIT_IN_PLACE || (side != 0 && side != 1) || (flip != 0 && flip != 1)) status = 5;
    /* (every contig id is below Glob.next_cid, which sized the masks: anything else is a bin out of range) */
    else if (st.cid[fb] < 0 || st.cid[fb] >= mask_n || (anchor >= 0 && (st.cid[anchor] < 0 || st.cid[anchor] >= mask_n))) status = 1;
    p.status = status;
    if (status) {
        plan[e] = p;
        return;
    }
    p.cs = st.cid[fb];
    p.a = st.pos[fb];
    p.b = st.pos[lb];
    p.n = p.b - p.a + 1;
    p.sp_a = st.spos[fb];
    p.sp_end = st.spos[lb] + st.sl[lb];
    p.bp_a = st.sbp[fb];
    p.bp_end = st.sbp[lb] + st.lb[lb];
    const int n_sub = p.sp_end - p.sp_a, n_bp = p.bp_end - p.bp_a;
    p.cut_prev = st.prev[fb];
    p.cut_next = st.next[lb];
    p.rem_L = st.L[fb] - p.n;
    p.rem_SL = st.SL[fb] - n_sub;
    p.rem_LB = st.LB[fb] - n_bp;
    if (anchor == EDIT_IN_PLACE) {
        p.cd = p.cs;
        p.same = 1;
        p.r = p.a;
        p.ins_sub = p.sp_a;
        p.ins_bp = p.bp_a;
        p.lnb = p.cut_prev;
        p.rnb = p.cut_next;
    } else if (anchor == EDIT_NEW_CONTIG) {
        p.cd = g->next_cid;
        p.same = 0;
        p.lnb = p.rnb = -1;
    } else {
        p.cd = st.cid[anchor];
        p.same = p.cd == p.cs;
        const int pa = st.pos[anchor];
        const bool behind = p.same && pa > p.b; /* the anchor lies behind the segment in its own contig: it moves up */
        const int ra = behind ? pa - p.n : pa;
        const int rsub = behind ? st.spos[anchor] - n_sub : st.spos[anchor];
        const int rbp = behind ? st.sbp[anchor] - n_bp : st.sbp[anchor];
        /* the anchor's neighbours in the order without the segment */
        const int an = (st.next[anchor] == fb) ? p.cut_next : st.next[anchor];
        const int ap = (st.prev[anchor] == lb) ? p.cut_prev : st.prev[anchor];
        if (side == 0) {
            p.r = ra + 1;
            p.ins_sub = rsub + st.sl[anchor];
            p.ins_bp = rbp + st.lb[anchor];
            p.lnb = anchor;
            p.rnb = an;
        } else {
            p.r = ra;
            p.ins_sub = rsub;
            p.ins_bp = rbp;
            p.lnb = ap;
            p.rnb = anchor;
        }
    }
    if (p.same) {
        p.dst_L = st.L[fb];
        p.dst_SL = st.SL[fb];
        p.dst_LB = st.LB[fb];
    } else if (anchor == EDIT_NEW_CONTIG) {
        p.dst_L = p.n;
        p.dst_SL = n_sub;
        p.dst_LB = n_bp;
    } else {
        p.dst_L = st.L[anchor] + p.n;
        p.dst_SL = st.SL[anchor] + n_sub;
        p.dst_LB = st.LB[anchor] + n_bp;
    }
    plan[e] = p;
    atomicOr(&mask[p.cs], 1ull << e);
    if (anchor >= 0) atomicOr(&mask[p.cd], 1ull << e);
}

/* grid (N / EDIT_THREADS, E): the dynamic arrays of bin f in the scratch state of edit blockIdx.y: dyn[e][k][N], k in the order of
 * State (pos, spos, cid, sbp, circ, prev, next, L, SL, LB, ori).  A refused edit's state is the current one. */
__global__ void __launch_bounds__(EDIT_THREADS) k_edit_state(State st, const EditPlan* __restrict__ plan, int N, int* __restrict__ dyn)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= N) return;
    const EditPlan p = plan[blockIdx.y];
    int pos = st.pos[f], spos = st.spos[f], cid = st.cid[f], sbp = st.sbp[f], prev = st.prev[f], next = st.next[f];
    int L = st.L[f], SL = st.SL[f], LB = st.LB[f], ori = st.ori[f];
    const int circ = st.circ[f];
    if (p.status == 0) {
        const int n_sub = p.sp_end - p.sp_a, n_bp = p.bp_end - p.bp_a;
        if (cid == p.cs && pos >= p.a && pos <= p.b) { /* in the segment */
            const int sl = st.sl[f], lb = st.lb[f];
            const int off = p.flip ? p.b - pos : pos - p.a;
            const int soff = p.flip ? p.sp_end - (spos + sl) : spos - p.sp_a;
            const int boff = p.flip ? p.bp_end - (sbp + lb) : sbp - p.bp_a;
            const int before = p.flip ? next : prev, behind = p.flip ? prev : next; /* inside the segment */
            prev = off > 0 ? before : p.lnb;
            next = off < p.n - 1 ? behind : p.rnb;
            pos = p.r + off;
            spos = p.ins_sub + soff;
            sbp = p.ins_bp + boff;
            cid = p.cd;
            L = p.dst_L;
            SL = p.dst_SL;
            LB = p.dst_LB;
            if (p.flip) ori = -ori;
        } else {
            if (cid == p.cs) { /* the remainder closes up */
                if (pos > p.b) {
                    pos -= p.n;
                    spos -= n_sub;
                    sbp -= n_bp;
                }
                if (prev == p.last) prev = p.cut_prev;
                if (next == p.first) next = p.cut_next;
                L = p.rem_L;
                SL = p.rem_SL;
                LB = p.rem_LB;
            }
            if (cid == p.cd) { /* the destination opens up */
                if (pos >= p.r) {
                    pos += p.n;
                    spos += n_sub;
                    sbp += n_bp;
                }
                if (f == p.rnb) prev = p.flip ? p.first : p.last;
                if (f == p.lnb) next = p.flip ? p.last : p.first;
                L = p.dst_L;
                SL = p.dst_SL;
                LB = p.dst_LB;
            }
        }
    }
    int* d = dyn + (size_t)blockIdx.y * NDYN * (size_t)N + f;
    const size_t n = (size_t)N;
    d[0] = pos;
    d[n] = spos;
    d[2 * n] = cid;
    d[3 * n] = sbp;
    d[4 * n] = circ;
    d[5 * n] = prev;
    d[6 * n] = next;
    d[7 * n] = L;
    d[8 * n] = SL;
    d[9 * n] = LB;
    d[10 * n] = ori;
}

/* the edits of the chunk that touch contig `cid` */
__device__ __forceinline__ unsigned long long edit_mask_of(const unsigned long long* __restrict__ mask, int mask_n, int cid)
{
    return (unsigned)cid < (unsigned)mask_n ? mask[cid] : 0ull;
}

/* the scratch tables of the chunk, edit e at offset e * M of each array */
struct EditTabs {
    float *dist, *stot;
    int* len;
    int2* cp;
};
__host__ __device__ inline Tables edit_tables(const EditTabs& t, int e, int M)
{
    Tables r;
    r.dist = t.dist + (size_t)e * M;
    r.stot = t.stot + (size_t)e * M;
    r.len = t.len + (size_t)e * M;
    r.cp = t.cp + (size_t)e * M;
    return r;
}

/* a workgroup's accumulators of one pass: EDIT_CHUNK edits x `W` words in LDS, flushed with one global atomic per word the workgroup
 * touched */
template <int W>
__device__ __forceinline__ void edit_flush(long long (*acc)[W], const unsigned long long* touched, long long* __restrict__ out, int w0)
{
    __syncthreads();
    const unsigned long long t = *touched;
    for (int i = threadIdx.x; i < EDIT_CHUNK * W; i += blockDim.x) {
        const int e = i / W, w = i % W;
        if (((t >> e) & 1ull) && acc[e][w]) atomic_add_ll(&out[e * EDIT_ACC + w0 + w], acc[e][w]);
    }
}

/* ONE pass over the contacts for the chunk: a contact whose two contigs no edit touches is done after two loads; any other is
 * evaluated once under the live coordinates and once under the tables of every edit whose bit is set: new - old -> out[e][0..1] */
__global__ void __launch_bounds__(EDIT_THREADS) k_edit_delta(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z, Tables tab, EditTabs et, int M,
                                                             const unsigned long long* __restrict__ mask, int mask_n, const Glob* g,
                                                             const double* __restrict__ lgf_tab, PzTab pz, long long* __restrict__ out)
{
    __shared__ long long acc[EDIT_CHUNK][2];
    __shared__ unsigned long long touched;
    for (int i = threadIdx.x; i < EDIT_CHUNK * 2; i += blockDim.x) (&acc[0][0])[i] = 0;
    if (threadIdx.x == 0) touched = 0ull;
    __syncthreads();
    const ig_params p = g->par[0];
    const ig_hot hot = ig_hot_make(p, ig_tab());
    const float mean = g->mean_kb;
    const ColMeta cm[2] = {{0.0f, 0}, {0.0f, 0}}; /* every contig an edit touches is linear, before and behind it */
    unsigned long long mine = 0ull;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < Z; k += (long long)gridDim.x * blockDim.x) {
        const int i = crow[k];
        const int2 v = cc[k];
        const int2 ci = tab.cp[i], cj = tab.cp[v.x];
        unsigned long long m = edit_mask_of(mask, mask_n, ci.x) | edit_mask_of(mask, mask_n, cj.x);
        if (!m) continue;
        const double lgf = lgfact_dev(v.y, lgf_tab);
        const long long q0 = eval_q(p, hot, mean, make_uint2(__float_as_uint(tab.dist[i]), (unsigned)ci.y),
                                    make_uint2(__float_as_uint(tab.dist[v.x]), (unsigned)cj.y | (ci.x == cj.x ? 0u : 1u << 28)), cm, v.y, lgf, pz, ig_tab());
        mine |= m;
        while (m) {
            const int e = __ffsll((long long)m) - 1;
            m &= m - 1;
            const size_t o = (size_t)e * M;
            const int2 ei = et.cp[o + i], ej = et.cp[o + v.x];
            const long long q1 = eval_q(p, hot, mean, make_uint2(__float_as_uint(et.dist[o + i]), (unsigned)ei.y),
                                        make_uint2(__float_as_uint(et.dist[o + v.x]), (unsigned)ej.y | (ei.x == ej.x ? 0u : 1u << 28)), cm, v.y, lgf, pz, ig_tab());
            if (q1 != q0) {
                atomic_add_ll(&acc[e][0], (q1 >> 32) - (q0 >> 32));
                atomic_add_ll(&acc[e][1], (long long)(unsigned int)q1 - (long long)(unsigned int)q0);
            }
        }
    }
    if (mine) atomicOr(&touched, mine);
    edit_flush<2>(acc, &touched, out, 0);
}

/* the same for the zero-pixel term and the intra pair count, over the sub-fragments whose contig an edit touches -> out[e][2..4] */
__global__ void __launch_bounds__(EDIT_THREADS) k_edit_zero_delta(Tables tab, EditTabs et, int M, const unsigned long long* __restrict__ mask, int mask_n,
                                                                  const Glob* g, const float* __restrict__ pz, int pz_n, long long* __restrict__ out)
{
    __shared__ long long acc[EDIT_CHUNK][3];
    __shared__ unsigned long long touched;
    for (int i = threadIdx.x; i < EDIT_CHUNK * 3; i += blockDim.x) (&acc[0][0])[i] = 0;
    if (threadIdx.x == 0) touched = 0ull;
    __syncthreads();
    const ig_params p = g->par[0];
    const float mean = g->mean_kb;
    unsigned long long mine = 0ull;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < M; s += gridDim.x * blockDim.x) {
        const int2 c0 = tab.cp[s];
        unsigned long long m = edit_mask_of(mask, mask_n, c0.x);
        if (!m) continue;
        const int len0 = tab.len[s];
        const long long q0 = c0.y > 0 ? zero_q(p, c0.y, len0, tab.stot[s], mean, pz, pz_n) : 0;
        const long long n0 = c0.y == 0 ? ((long long)len0 * (long long)(len0 - 1)) / 2 : 0;
        mine |= m;
        while (m) {
            const int e = __ffsll((long long)m) - 1;
            m &= m - 1;
            const size_t o = (size_t)e * M + s;
            const int pos = et.cp[o].y, len = et.len[o];
            const long long q1 = pos > 0 ? zero_q(p, pos, len, et.stot[o], mean, pz, pz_n) : 0;
            const long long n1 = pos == 0 ? ((long long)len * (long long)(len - 1)) / 2 : 0;
            if (q1 != q0) {
                atomic_add_ll(&acc[e][0], (q1 >> 32) - (q0 >> 32));
                atomic_add_ll(&acc[e][1], (long long)(unsigned int)q1 - (long long)(unsigned int)q0);
            }
            if (n1 != n0) atomic_add_ll(&acc[e][2], n1 - n0);
        }
    }
    if (mine) atomicOr(&touched, mine);
    edit_flush<3>(acc, &touched, out, 2);
}

/* ig_edit_apply: the dynamic arrays of the scratch state of edit 0 become the live ones, the id of a new contig is used up, the stale
 * insert flags are cleared (as ig_upload_state does) */
__global__ void k_edit_commit(State st, const int* __restrict__ dyn, int N, Glob* g, int new_contig)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f == 0) {
        if (new_contig) g->next_cid += 1;
        for (int i = 0; i < 12; i++) g->valid_insert[i] = 0;
    }
    if (f >= N) return;
    const size_t n = (size_t)N;
    st.pos[f] = dyn[f];
    st.spos[f] = dyn[n + f];
    st.cid[f] = dyn[2 * n + f];
    st.sbp[f] = dyn[3 * n + f];
    st.circ[f] = dyn[4 * n + f];
    st.prev[f] = dyn[5 * n + f];
    st.next[f] = dyn[6 * n + f];
    st.L[f] = dyn[7 * n + f];
    st.SL[f] = dyn[8 * n + f];
    st.LB[f] = dyn[9 * n + f];
    st.ori[f] = dyn[10 * n + f];
}
