/* ig_kernels_junc.cuh -- the junction support profile of the current genome: for every junction j between the positions j - 1 and j
 * of the genome order (the contact map's positions) the contacts that span it inside a window of w positions, the sub-fragment
 * pairs that could, and what the model in use expects of them.  The rule is stated once, in instagraal_amd/junction_profile.py;
 * the kernels here reproduce it entry for entry.
 *
 * Everything is a DIFFERENCE array of T + 1 64-bit words that a prefix sum turns into the profile: a pair (pa, pb), pa < pb, of one
 * placed contig that is not a ring adds its value at word pa + 1 and takes it away at word pb + 1, so the junctions pa < j <= pb
 * see it.  Unsigned wrap-around adds: the sums return to 0 behind every contig, so whatever wraps on the way unwraps again, and
 * integer addition makes the result independent of threads, waves, workgroups and the order of the atomics.  The records are
 * the genome view's (ig_kernels_genome.cuh), the prefix sum is the 64-bit scan of ig_kernels_rows.cuh.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define JUNC_THREADS 256
#define JUNC_MAX_WINDOW 1024
#define JUNC_NS 8 /* scalars: the order of ig_junction_profile's scalars[8] */
#define JUNC_IN_OBS 0
#define JUNC_BEYOND_OBS 1
#define JUNC_TRANS_OBS 2
#define JUNC_RING_OBS 3
#define JUNC_UNPLACED_OBS 4
#define JUNC_N_OBS 5 /* (the words the observed pass owns) */
#define JUNC_INTERNAL 5
#define JUNC_SPANNED 6  /* (summed on the host from the profile) */
#define JUNC_DEV_MAXQ 6 /* on the device that word holds the largest |quantised model value| the model pass saw */
#define JUNC_WAVE_WINDOW 64 /* windows beyond this: one wave per position in the model pass, else one thread */

/* The observed part: one pass over the contacts (row of contact k: crow[k]; column and count: cc[k]; row-major sorted), one
 * 16-byte record gather per end as k_law_observed.  An in-window contact adds +c at word pa + 1 and -c at word pb + 1.
 *
 * COMBINE = false, the yardstick: one atomic per end.
 *
 * COMBINE = true: the lanes of a wave hold 64 consecutive contacts, mostly of one row, whose + ends are then ONE word: equal +
 * destinations next to each other are summed inside the wave first (wave_runs and wave_run_sum, ig_kernels_wave.cuh) and only
 * the head of a run issues the atomic.  The - ends are neighbouring words and go out as they are.
 * V: int where 64 counts cannot overflow one, else long long.
 *
 * The five classes of contact are summed in registers and reach memory once per workgroup.  A sharded handle takes the rows
 * i % world == rank: the ranks' difference arrays, and so their profiles, add up. */
template <bool COMBINE, typename V>
__global__ void __launch_bounds__(JUNC_THREADS) k_junc_observed(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                                const int4* __restrict__ rec, int window, unsigned long long* __restrict__ diff,
                                                                unsigned long long* __restrict__ out_sc, int rank, int world)
{
    __shared__ unsigned long long sc[JUNC_N_OBS];
    class_zero<JUNC_N_OBS>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_in = 0, r_beyond = 0, r_trans = 0, r_ring = 0, r_unpl = 0;
    const long long stride = (long long)gridDim.x * JUNC_THREADS;
    const long long Zr = (Z + 63) & ~63LL; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * JUNC_THREADS + threadIdx.x; k < Zr; k += stride) {
        int plus = -1, minus = -1; /* the words of the two ends, -1: not an in-window contact */
        unsigned long long cv = 0;
        if (k < Z) {
            const int i = crow[k];
            if (contact_is_mine(i, rank, world)) {
                const int2 e = cc[k];
                const int4 a = rec[i], b = rec[e.x];
                cv = (unsigned long long)(long long)e.y;
                const GenomePair cls = genome_pair_class(a, b);
                if (cls == PAIR_UNPLACED) r_unpl += cv;
                else if (cls == PAIR_TRANS) r_trans += cv;
                else if (cls == PAIR_RING) r_ring += cv;
                else {
                    const int pa = min(a.w, b.w), pb = max(a.w, b.w);
                    if (pb - pa <= window) {
                        r_in += cv;
                        plus = pa + 1;
                        minus = pb + 1;
                    } else
                        r_beyond += cv;
                }
            }
        }
        if (minus >= 0) atomicAdd(&diff[minus], 0ull - cv);
        if (!COMBINE) {
            if (plus >= 0) atomicAdd(&diff[plus], cv);
            continue;
        }
        V v = plus >= 0 ? (V)(long long)cv : (V)0;
        const WaveRuns runs = wave_runs(plus, lane);
        v = wave_run_sum<V>(runs, v, lane);
        if (runs.head && plus >= 0 && v != 0) atomicAdd(&diff[plus], (unsigned long long)(long long)v);
    }
    if (r_in) atomicAdd(&sc[JUNC_IN_OBS], r_in);
    if (r_beyond) atomicAdd(&sc[JUNC_BEYOND_OBS], r_beyond);
    if (r_trans) atomicAdd(&sc[JUNC_TRANS_OBS], r_trans);
    if (r_ring) atomicAdd(&sc[JUNC_RING_OBS], r_ring);
    if (r_unpl) atomicAdd(&sc[JUNC_UNPLACED_OBS], r_unpl);
    class_flush<JUNC_N_OBS>(sc, out_sc);
}

/* the internal junctions: positions of a placed contig that is not a ring, its first left out */
__global__ void __launch_bounds__(JUNC_THREADS) k_junc_count(const int2* __restrict__ meta, int T, unsigned long long* __restrict__ out_internal)
{
    __shared__ unsigned int n;
    if (threadIdx.x == 0) n = 0;
    __syncthreads();
    const int r = blockIdx.x * JUNC_THREADS + threadIdx.x;
    bool internal = false;
    if (r < T) {
        const int2 m = meta[r];
        internal = m.y > 0 && r > max(m.x, 0);
    }
    const unsigned long long b = __ballot(internal);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n, (unsigned int)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && n) atomicAdd(out_internal, (unsigned long long)n);
}

/* The model part, no atomics on the arrays.  With q(i, k) = ig_quantize((double) ig_rippe(fabsf(dist_i - dist_k), p)) under the
 * parameter set the moves are scored under, position r of a placed contig [start, end) that is not a ring owns the pairs it opens,
 * A[r] = sum of q(r, k) over k = r + 1 .. min(r + w, end - 1), and the pairs it closes, B[r] = sum of q(i, r) over
 * i = max(r - w, start) .. r - 1; its difference word r + 1 is A[r] - B[r] (and the number of the ones minus the number of the
 * others for the pairs), so expected_q[j] = sum over t < j of A[t] - B[t].
 *
 * G lanes share a position: G = 64, a wave with an integer wave reduction, for windows of hundreds; G = 1, a thread, for small
 * ones.  Integer sums: the result is the same either way.  *maxq takes the largest |q| seen (the host's overflow guard). */
template <int G>
__global__ void __launch_bounds__(JUNC_THREADS) k_junc_model(const float* __restrict__ ds, const int2* __restrict__ meta, int T, int window,
                                                             const Glob* __restrict__ g, unsigned long long* __restrict__ d_pairs,
                                                             unsigned long long* __restrict__ d_exp, unsigned long long* __restrict__ maxq)
{
    const int r = (int)(((long long)blockIdx.x * JUNC_THREADS + threadIdx.x) / G);
    const int sub = threadIdx.x % G;
    const bool live = r < T;
    const ig_params p = g->par[0];
    unsigned long long acc = 0, n_pairs = 0, mx = 0;
    if (live) {
        const int2 m = meta[r];
        if (m.y > 0) {
            const int start = max(m.x, 0);
            const int end = min(start + m.y, T);
            const int hi = min(r + window, end - 1); /* the last k in front */
            const int lo = max(r - window, start);   /* the first i behind */
            const int nf = max(hi - r, 0), nb = max(r - lo, 0);
            n_pairs = (unsigned long long)(long long)(nf - nb);
            const float dr = ds[r];
            for (int o = sub; o < nf + nb; o += G) {
                const int other = o < nf ? r + 1 + o : lo + (o - nf);
                const long long q = ig_quantize((double)ig_rippe(fabsf(dr - ds[other]), p, ig_tab()));
                acc += o < nf ? (unsigned long long)q : 0ull - (unsigned long long)q;
                const unsigned long long aq = (unsigned long long)(q < 0 ? -q : q);
                mx = aq > mx ? aq : mx;
            }
        }
    }
    /* (one loop for the maximum and the sum: their shuffles interleave; wave_max_u64 behind wave_sum_u64 measured slower) */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
        if (G == 64) acc += __shfl_xor(acc, d, 64);
    }
    if (live && sub == 0) {
        d_pairs[r + 1] = n_pairs;
        d_exp[r + 1] = acc;
        if (r == 0) {
            d_pairs[0] = 0ull;
            d_exp[0] = 0ull;
        }
    }
    if ((threadIdx.x & 63) == 0) raise_max(maxq, mx);
}
