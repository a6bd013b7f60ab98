/* ig_kernels_cutjoin.cuh -- cut and join scores (the rule: instagraal_amd/cut_join.py): the part of the likelihood change of EVERY
 * cut of a linear contig and of EVERY link of two linear contigs that has a closed structure, as exact integers in the units of the
 * exact scorer (ig_kernels_edit.cuh), from one pass over the contacts each.
 *
 * Both passes over the contacts take one contact per thread and one 16-byte record per end (k_cj_sub_records, k_cj_bin_records); the
 * trans term, which depends on the count alone, is cj_trans_q on constants the host forms with the functions of ig_detmath.h.  No
 * kernel here uses scratch or spills a register (the table: DESIGN.md 4.24).
 *
 * Cuts.  A cis contact of a linear contig whose two bins differ changes its term from cis to trans under every cut between the two
 * bins: d = trans term - eval_q(live) goes into a DIFFERENCE array over the bins in a layout where a contig's bins lie next to
 * each other in their order (slot = first slot of the contig + pos; the host numbers the contigs), +d at the word behind the earlier
 * bin and -d at the word behind the later one, in three arrays: the hi limbs, the lo limbs, the contacts.  The 64-bit scan of
 * ig_kernels_rows.cuh turns them into the sums per junction; every contribution closes inside its contig, so one unsegmented scan
 * does, and whatever wraps on the way unwraps again.  Contacts arrive sorted by row: the words of the row's end repeat along a wave
 * and are summed inside it first (wave_runs, wave_run_sum), the other end goes out as it is.
 * The zero-pixel sum of a linear contig of L sub-fragments, G(L) = sum over pos = 1 .. L - 1 of zero_q(pos, L), is what the z limbs
 * of a cut (G(j) + G(L - j) - G(L)) and of a link (G(La + Lb) - G(La) - G(Lb)) are made of.  Beyond the first rank p* with
 * (float) p* x mean_kb >= d_max a term is quantize(-(v_inter x (L - pos))), whose sums over pos do not depend on L: they are read
 * from a prefix table (k_cj_vk and the scan), the ranks below p* are evaluated, a wave per sum.
 *
 * Links.  The pairs of linear contigs with a contact between them are the rows of the shared row builder (k_cj_pairs_emit: row a,
 * word b << 32 | 1, reduced: CSR over the contigs with the contacts per pair).  Then one pass over the contacts (k_cj_join): a trans
 * contact between linear contigs finds its pair by binary search in row a, evaluates the trans term once and the cis term under the
 * coordinates each of the four links (sa, sb) would give its two sub-fragments -- computed here from sbp, len_bp, LB, SL and the
 * SubTab with exactly the operations of k_fill_tables -- and adds eight limbs, in one of two forms with the same bytes: accumulators
 * in LDS per workgroup for a window of CJ_LDS_PAIRS pairs, flushed with one atomic per non-zero word; or global atomics behind a
 * wave-run aggregation by pair.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define CJ_THREADS 256
#define CJ_LDS_PAIRS 256 /* pairs whose eight words a workgroup keeps in LDS: 16 KiB, so that LDS does not limit the waves of a CU */
#define CJ_ARR_HI 0
#define CJ_ARR_LO 1
#define CJ_ARR_CNT 2
#define CJ_ARRAYS 3

/* the prefix table of the zero-pixel terms beyond p*: T_hi[n], T_lo[n] = the limbs of sum over k = 1 .. n of quantize(-(v_inter k)) */
struct CjZeroTab {
    const long long *hi, *lo;
    int pstar; /* first rank whose separation is not below d_max (>= 1) */
};

/* The trans term of a contact of count ob, which depends on the count alone: eval_q's trans branch with what does not depend on the
 * contact formed once, on the host, by the functions of ig_detmath.h (cj_trans_const, ig_host_cutjoin.inc) -- the same doubles on
 * both sides.  fast: ig_term_hot(0, inter, ..) = (fma(ob, lg, -ex) - lgf) + vz with lg = log2(v_inter) log10(2), ex = 2^log2(v_inter);
 * else ig_pixel_term(v_inter, v_inter, ..) with e = v_inter, l10 = log10(e).  vz = v_inter x the float log10(e) of the kernels. */
struct CjTrans {
    double lg, ex, vz, e, l10;
    int fast, pad;
};
__device__ __forceinline__ long long cj_trans_q(const CjTrans& c, int ob, double lgf)
{
    double t;
    if (c.fast && ob > 0) {
        t = (ig_fma((double)ob, c.lg, -c.ex) - lgf) + c.vz;
    } else {
        double res = 0.0;
        if (c.e != 0.0) res = ob > 0 ? ((double)ob * c.l10 - c.e) - lgf : -c.e;
        t = res + c.vz;
    }
    return ig_quantize(t);
}

/* one 16-byte record per sub-fragment, one gather per contact endpoint in k_cut_span: (dist, contig, rank, slot of its bin or -1: a ring) */
__global__ void __launch_bounds__(CJ_THREADS) k_cj_sub_records(Tables t, const SubTab* __restrict__ sub, const int* __restrict__ slotl, int M, int4* __restrict__ rec)
{
    const int s = blockIdx.x * CJ_THREADS + threadIdx.x;
    if (s >= M) return;
    const int2 cp = t.cp[s];
    rec[s] = make_int4(__float_as_int(t.dist[s]), cp.x, cp.y, slotl[sub[s].parent]);
}

/* two 16-byte records per bin, what k_cj_join needs of the state: (sbp, spos, sl, lb), (ori, LB, SL, the number of its contig among the
 * linear ones or -1) */
__global__ void __launch_bounds__(CJ_THREADS) k_cj_bin_records(State st, const int* __restrict__ kof, int N, int4* __restrict__ rec)
{
    const int f = blockIdx.x * CJ_THREADS + threadIdx.x;
    if (f >= N) return;
    rec[2 * (size_t)f] = make_int4(st.sbp[f], st.spos[f], st.sl[f], st.lb[f]);
    rec[2 * (size_t)f + 1] = make_int4(st.ori[f], st.LB[f], st.SL[f], kof[f]);
}

/* ONE pass over the contacts: the three difference arrays of the cuts (stride words apart), from the records of k_cj_sub_records */
__global__ void __launch_bounds__(CJ_THREADS) k_cut_span(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z, const int4* __restrict__ rec,
                                                         const Glob* g, const double* __restrict__ lgf_tab, PzTab pz, CjTrans tc,
                                                         unsigned long long* __restrict__ diff, long long stride)
{
    const ig_params p = g->par[0];
    const ig_hot hot = ig_hot_make(p, ig_tab());
    const float mean = g->mean_kb;
    const ColMeta cm[2] = {{0.0f, 0}, {0.0f, 0}}; /* linear contigs only */
    const int lane = threadIdx.x & 63;
    { /* one contact per thread: whole waves reach the shuffles together (the grid covers Z rounded up to workgroups) */
        const long long k = (long long)blockIdx.x * CJ_THREADS + threadIdx.x;
        int own = -1, other = -1; /* the words of the row's end and of the column's, -1: not a spanning contact */
        long long dh = 0, dl = 0, dc = 0;
        int4 a = make_int4(0, -1, 0, -1), b = make_int4(0, -2, 0, -1);
        int ob = 0;
        if (k < Z) {
            const int2 v = cc[k];
            a = rec[crow[k]];
            b = rec[v.x];
            ob = v.y;
        }
        if (a.y == b.y && a.w >= 0 && b.w >= 0 && a.w != b.w) { /* one linear contig, two bins */
            const double lgf = lgfact_dev(ob, lgf_tab);
            const long long q0 = eval_q(p, hot, mean, make_uint2((unsigned)a.x, (unsigned)a.z & 0x0fffffffu), make_uint2((unsigned)b.x, (unsigned)b.z & 0x0fffffffu), cm, ob, lgf,
                                         pz, ig_tab()); /* (the masks: both ends carry code 0 of cm, known to the compiler) */
            const long long q1 = cj_trans_q(tc, ob, lgf);
            const long long sgn = a.w < b.w ? 1 : -1; /* + behind the earlier bin, - behind the later one */
            dh = sgn * ((q1 >> 32) - (q0 >> 32));
            dl = sgn * ((long long)(unsigned int)q1 - (long long)(unsigned int)q0);
            dc = sgn;
            own = a.w + 1;
            other = b.w + 1;
        }
        if (other >= 0) {
            if (dh) atomicAdd(&diff[CJ_ARR_HI * stride + other], (unsigned long long)(0 - dh));
            if (dl) atomicAdd(&diff[CJ_ARR_LO * stride + other], (unsigned long long)(0 - dl));
            atomicAdd(&diff[CJ_ARR_CNT * stride + other], (unsigned long long)(0 - dc));
        }
        const WaveRuns runs = wave_runs(own, lane);
        dh = wave_run_sum<long long>(runs, dh, lane);
        dl = wave_run_sum<long long>(runs, dl, lane);
        dc = wave_run_sum<long long>(runs, dc, lane);
        if (runs.head && own >= 0) {
            if (dh) atomicAdd(&diff[CJ_ARR_HI * stride + own], (unsigned long long)dh);
            if (dl) atomicAdd(&diff[CJ_ARR_LO * stride + own], (unsigned long long)dl);
            if (dc) atomicAdd(&diff[CJ_ARR_CNT * stride + own], (unsigned long long)dc);
        }
    }
}

/* a[k] = the limbs of quantize(-(v_inter k)), k = 0 .. n - 1 (a[0] = 0): zero_q's value beyond d_max at L - pos = k */
__global__ void __launch_bounds__(CJ_THREADS) k_cj_vk(const Glob* g, int n, unsigned long long* __restrict__ a_hi, unsigned long long* __restrict__ a_lo)
{
    const int k = blockIdx.x * CJ_THREADS + threadIdx.x;
    if (k >= n) return;
    const long long q = k ? ig_quantize(0.0 - ((double)g->par[0].v_inter * (double)k)) : 0;
    a_hi[k] = (unsigned long long)(q >> 32);
    a_lo[k] = (unsigned long long)(long long)(unsigned int)q;
}

/* this lane's share of sgn x G(L): the ranks below p* evaluated, the rest (lane 0) from the table.  Whole waves call; the caller sums
 * hi and lo over the wave */
__device__ __forceinline__ void cj_G_lane(const ig_params& p, float mean, const float* __restrict__ pz, int pz_n, const CjZeroTab& zt, int L, long long sgn,
                                          int lane, long long& hi, long long& lo)
{
    const int end = min(L, zt.pstar);
    for (int pos = 1 + lane; pos < end; pos += 64) {
        const long long q = zero_q(p, pos, L, 0.0f, mean, pz, pz_n);
        hi += sgn * (q >> 32);
        lo += sgn * (long long)(unsigned int)q;
    }
    if (lane == 0 && L > zt.pstar) {
        hi += sgn * zt.hi[L - zt.pstar];
        lo += sgn * zt.lo[L - zt.pstar];
    }
}

/* a wave per linear contig k: G of its sub-fragments -> gc[k], gc[K + k].  csl[k]: its sub-fragments */
__global__ void __launch_bounds__(CJ_THREADS) k_cj_contig_zero(const int* __restrict__ csl, int K, const Glob* g, const float* __restrict__ pz, int pz_n, CjZeroTab zt,
                                                               long long* __restrict__ gc)
{
    const int k = (int)(((long long)blockIdx.x * CJ_THREADS + threadIdx.x) >> 6);
    if (k >= K) return;
    const int lane = threadIdx.x & 63;
    long long hi = 0, lo = 0;
    cj_G_lane(g->par[0], g->mean_kb, pz, pz_n, zt, csl[k], 1, lane, hi, lo);
    hi = wave_sum_ll(hi);
    lo = wave_sum_ll(lo);
    if (lane == 0) {
        gc[k] = hi;
        gc[(size_t)K + k] = lo;
    }
}

/* a wave per bin f: the z limbs of the cut in front of it, G(j) + G(L - j) - G(L) -> out[f], out[N + f]; 0 where no cut exists.  G(L)
 * is the contig's, formed once by k_cj_contig_zero (gc, K; kof[f]: the number of the bin's contig); the two halves depend on the bin */
__global__ void __launch_bounds__(CJ_THREADS) k_cut_zero(State st, const int* __restrict__ kof, int N, const long long* __restrict__ gc, int K, const Glob* g,
                                                         const float* __restrict__ pz, int pz_n, CjZeroTab zt, long long* __restrict__ out)
{
    const int f = (int)(((long long)blockIdx.x * CJ_THREADS + threadIdx.x) >> 6);
    if (f >= N) return; /* (the whole wave) */
    const int lane = threadIdx.x & 63;
    long long hi = 0, lo = 0;
    const int k = kof[f];
    if ((unsigned)k < (unsigned)K && st.prev[f] >= 0) {
        const ig_params p = g->par[0];
        const float mean = g->mean_kb;
        const int j = st.spos[f], L = st.SL[f];
        cj_G_lane(p, mean, pz, pz_n, zt, j, 1, lane, hi, lo);
        cj_G_lane(p, mean, pz, pz_n, zt, L - j, 1, lane, hi, lo);
        if (lane == 0) {
            hi -= gc[k];
            lo -= gc[(size_t)K + k];
        }
    }
    hi = wave_sum_ll(hi);
    lo = wave_sum_ll(lo);
    if (lane == 0) {
        out[f] = hi;
        out[(size_t)N + f] = lo;
    }
}

/* ---- links */

/* The pairs: one pass over the contacts, twice (the counting sort of the row builder).  kof[f]: the number of bin f's contig among
 * the linear ones, -1: a ring.  A trans contact between linear contigs a < b is an entry (row a, word b << 32 | 1). */
template <bool SCATTER>
__global__ void __launch_bounds__(CJ_THREADS) k_cj_pairs_emit(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                              const SubTab* __restrict__ sub, const int* __restrict__ kof, unsigned long long* __restrict__ counter,
                                                              unsigned long long* __restrict__ ent, unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[1];
    if (!SCATTER) class_zero<1>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_ent = 0;
    const long long step = (long long)gridDim.x * CJ_THREADS;
    const long long Zr = (Z + 63) & ~63LL;
    for (long long k = (long long)blockIdx.x * CJ_THREADS + threadIdx.x; k < Zr; k += step) {
        int lo = -1, hi = 0;
        if (k < Z) {
            const int ka = kof[sub[crow[k]].parent], kb = kof[sub[cc[k].x].parent];
            if (ka >= 0 && kb >= 0 && ka != kb) {
                lo = min(ka, kb);
                hi = max(ka, kb);
                r_ent += 1;
            }
        }
        const unsigned long long slot = rows_slot<SCATTER>(counter, lo, lane);
        if (SCATTER && lo >= 0 && slot < n_ent) ent[slot] = lift_pack(hi, 1);
    }
    if (SCATTER) return;
    if (r_ent) atomicAdd(&sc[0], r_ent);
    class_flush<1>(sc, out_sc);
}

/* the coordinates k_fill_tables would give sub-fragment b of a bin that starts at sbp / spos (sl sub-fragments) with orientation ori */
__device__ __forceinline__ uint2 cj_coord(const SubTab& b, int sbp, int spos, int sl, int ori)
{
    const float dfi = (ori == 1) ? b.wat : b.cri;
    const float dist = (float)sbp / 1000.0f + dfi;
    return make_uint2(__float_as_uint(dist), (unsigned)((ori == 1) ? spos + b.w : spos + (sl - 1) - b.w) & 0x0fffffffu); /* (code 0 of cm) */
}

/* ONE pass over the contacts: the eight limbs of every pair, acc[pair][2 (2 sa + sb) + {hi, lo}], sides 0: head, 1: tail.  The link
 * (sa, sb) keeps a and moves all of b: behind a's tail (sa = 1; b reversed where sb = 1) or in front of a's head (sa = 0; b reversed
 * where sb = 0).  LDS = true: the pairs p0 <= pair < p0 + CJ_LDS_PAIRS in LDS; LDS = false: every pair, atomics per run of a wave. */
template <bool LDS>
__global__ void __launch_bounds__(CJ_THREADS) k_cj_join(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z, const SubTab* __restrict__ sub,
                                                        const int4* __restrict__ brec, const unsigned long long* __restrict__ rowptr, const int* __restrict__ col,
                                                        int n_pairs, int p0, const Glob* g, const double* __restrict__ lgf_tab, PzTab pz, CjTrans tc,
                                                        long long* __restrict__ acc)
{
    __shared__ long long lacc[LDS ? CJ_LDS_PAIRS * 8 : 1];
    if (LDS) {
        for (int i = threadIdx.x; i < CJ_LDS_PAIRS * 8; i += CJ_THREADS) lacc[i] = 0;
        __syncthreads();
    }
    const ig_params p = g->par[0];
    const ig_hot hot = ig_hot_make(p, ig_tab());
    const float mean = g->mean_kb;
    const ColMeta cm[2] = {{0.0f, 0}, {0.0f, 0}};
    const int lane = threadIdx.x & 63;
    { /* one contact per thread: whole waves reach the shuffles together (the grid covers Z rounded up to workgroups) */
        const long long k = (long long)blockIdx.x * CJ_THREADS + threadIdx.x;
        long long pair = -1;
        SubTab sx = {0, 0.0f, 0.0f, 0}, sy = sx; /* sx: the end in a, the contig of the lower number */
        int4 a0 = make_int4(0, 0, 0, 0), a1 = make_int4(0, 0, 0, -1), b0 = a0, b1 = a1; /* their bins' records */
        int ob = 0;
        if (k < Z) {
            const int2 v = cc[k];
            sx = sub[crow[k]];
            sy = sub[v.x];
            ob = v.y;
            a0 = brec[2 * (size_t)sx.parent], a1 = brec[2 * (size_t)sx.parent + 1];
            b0 = brec[2 * (size_t)sy.parent], b1 = brec[2 * (size_t)sy.parent + 1];
        }
        if (a1.w >= 0 && b1.w >= 0 && a1.w != b1.w) {
            if (a1.w > b1.w) {
                const SubTab t = sx;
                sx = sy;
                sy = t;
                const int4 t0 = a0, t1 = a1;
                a0 = b0, a1 = b1;
                b0 = t0, b1 = t1;
            }
            /* the pair: b in row a */
            const long long end = (long long)rowptr[a1.w + 1];
            long long lo = (long long)rowptr[a1.w], hi = end;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (col[mid] < b1.w) lo = mid + 1;
                else hi = mid;
            }
            if (lo < end && col[lo] == b1.w && (!LDS || (lo >= p0 && lo < (long long)p0 + CJ_LDS_PAIRS))) pair = lo; /* (end <= n_pairs) */
        }
        const double lgf = lgfact_dev(ob, lgf_tab);
        const long long qt = cj_trans_q(tc, ob, lgf);
        WaveRuns runs;
        if (!LDS) runs = wave_runs(pair, lane);
        /* t = 2 sa + sb: the cis term of the link (sa, sb).  One instance of eval_q; whole waves stay together.
         * records: a0 / b0 = (sbp, spos, sl, lb), a1 / b1 = (ori, LB, SL, k) */
#pragma unroll
        for (int t = 0; t < 4; t++) {
            long long dh = 0, dl = 0;
            if (pair >= 0) {
                const int sa = t >> 1, sb = t & 1;
                const int flip = sa ? sb == 1 : sb == 0;
                const int ins_bp = sa ? a1.y : 0, ins_sub = sa ? a1.z : 0; /* where b starts */
                const uint2 ca = cj_coord(sx, sa ? a0.x : a0.x + b1.y, sa ? a0.y : a0.y + b1.z, a0.z, a1.x);
                const uint2 cb = flip ? cj_coord(sy, ins_bp + (b1.y - (b0.x + b0.w)), ins_sub + (b1.z - (b0.y + b0.z)), b0.z, -b1.x)
                                      : cj_coord(sy, ins_bp + b0.x, ins_sub + b0.y, b0.z, b1.x);
                const long long q = eval_q(p, hot, mean, ca, cb, cm, ob, lgf, pz, ig_tab());
                dh = (q >> 32) - (qt >> 32);
                dl = (long long)(unsigned int)q - (long long)(unsigned int)qt;
            }
            const int w = 2 * t;
            if (LDS) {
                if (dh) atomic_add_ll(&lacc[(pair - p0) * 8 + w], dh);
                if (dl) atomic_add_ll(&lacc[(pair - p0) * 8 + w + 1], dl);
            } else {
                dh = wave_run_sum<long long>(runs, dh, lane);
                dl = wave_run_sum<long long>(runs, dl, lane);
                if (runs.head && pair >= 0) {
                    if (dh) atomic_add_ll(&acc[pair * 8 + w], dh);
                    if (dl) atomic_add_ll(&acc[pair * 8 + w + 1], dl);
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < CJ_LDS_PAIRS * 8; i += CJ_THREADS)
            if (lacc[i] && (long long)p0 + i / 8 < n_pairs) atomic_add_ll(&acc[(long long)p0 * 8 + i], lacc[i]);
    }
}

/* a wave per pair (a, b): the z limbs of its links, G(La + Lb) - G(La) - G(Lb) -> zacc[pair][2] */
__global__ void __launch_bounds__(CJ_THREADS) k_cj_join_zero(const unsigned long long* __restrict__ rowptr, const int* __restrict__ col, long long n_pairs,
                                                             const int* __restrict__ csl, int K, const long long* __restrict__ gc, const Glob* g,
                                                             const float* __restrict__ pz, int pz_n, CjZeroTab zt, long long* __restrict__ zacc)
{
    const long long pr = ((long long)blockIdx.x * CJ_THREADS + threadIdx.x) >> 6;
    if (pr >= n_pairs) return;
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = K; /* the row: the last a with rowptr[a] <= pr */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)rowptr[mid] <= pr) lo = mid;
        else hi = mid;
    }
    const int a = lo, b = col[pr];
    long long zh = 0, zl = 0;
    if ((unsigned)b < (unsigned)K) cj_G_lane(g->par[0], g->mean_kb, pz, pz_n, zt, csl[a] + csl[b], 1, lane, zh, zl);
    zh = wave_sum_ll(zh);
    zl = wave_sum_ll(zl);
    if (lane == 0 && (unsigned)b < (unsigned)K) {
        zacc[pr * 2] = zh - gc[a] - gc[b];
        zacc[pr * 2 + 1] = zl - gc[(size_t)K + a] - gc[(size_t)K + b];
    }
}

/* tests: eval_q itself, ring-free, for contact k at separation s[k], rank distance d[k] (< 2^28), count ob[k]; trans[k] != 0: a trans
 * pair -- what ig_contact_terms_host restates on the host */
__global__ void __launch_bounds__(CJ_THREADS) k_debug_contact_terms(const float* __restrict__ s, const int* __restrict__ d, const int* __restrict__ trans,
                                                                    const int* __restrict__ ob, long long n, const Glob* g, const double* __restrict__ lgf_tab,
                                                                    PzTab pz, long long* __restrict__ q)
{
    const long long k = (long long)blockIdx.x * CJ_THREADS + threadIdx.x;
    if (k >= n) return;
    const ig_params p = g->par[0];
    const ig_hot hot = ig_hot_make(p, ig_tab());
    const ColMeta cm[2] = {{0.0f, 0}, {0.0f, 0}};
    q[k] = eval_q(p, hot, g->mean_kb, make_uint2(__float_as_uint(s[k]), (unsigned)d[k] & 0x0fffffffu), make_uint2(0u, trans[k] ? 1u << 28 : 0u), cm, ob[k],
                  lgfact_dev(ob[k], lgf_tab), pz, ig_tab());
}
