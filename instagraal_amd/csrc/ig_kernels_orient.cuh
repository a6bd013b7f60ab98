/* ig_kernels_orient.cuh -- orientation support: which segments of the current genome the contacts would reverse.  The caller gives
 * intervals [first, last] of positions of the genome order; the contacts between a segment's two ARMS (its outermost
 * m = min(n / 2, w) positions on either side) and its two FLANKS (the up to w positions of the contig on either side) are summed
 * in four quadrants LL, LR, RL, RR (arm, flank), next to what the model in use expects of the pairs that keep each arm with the flank
 * on its own side and of the pairs that would join it to the other.  The rule is stated once, in
 * instagraal_amd/orientation_support.py; the kernels here reproduce it byte for byte.
 *
 * Integer sums throughout: the result does not depend on threads, waves, workgroups or the order of the atomics.  The records,
 * ds and meta are the genome view's (ig_kernels_genome.cuh).
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define ORIENT_THREADS 256
#define ORIENT_NS 8 /* scalars: the order of ig_orientation_support's scalars[8] */
#define ORIENT_UNPLACED 0
#define ORIENT_TRANS 1
#define ORIENT_RING 2
#define ORIENT_WITHIN 3
#define ORIENT_COUNTED 4
#define ORIENT_UNCOUNTED 5
#define ORIENT_ENTRIES 6
#define ORIENT_N_OBS 7     /* (the words the observed pass owns) */
#define ORIENT_JUDGED 7    /* (counted on the host from the geometry) */
#define ORIENT_DEV_MAXQ 7  /* on the device that word holds the largest |quantised model value| the model pass saw */
#define ORIENT_WAVE_PAIRS 4096 /* segments with 2 * pairs beyond this: a workgroup per segment in the model pass, else a wave */
/* the quadrants: word 4 * segment + quadrant of the observed array */
#define ORIENT_LL 0
#define ORIENT_LR 1
#define ORIENT_RL 2
#define ORIENT_RR 3
/* the words of OrientBuf.ctl */
#define ORIENT_CTL_ERR 0   /* k_orient_segments: the list is malformed (bit 0 range, 1 order, 2 two contigs) */
#define ORIENT_CTL_LARGE 1 /* ... segments listed for the workgroup form of the model pass */

/* One thread per segment k: the list is checked -- in range, ascending and disjoint (against the segment in front), both ends in one
 * contig by meta -- and a malformed one sets the error word: the host fails loudly and nothing is written out of bounds.  geo[k] =
 * (status, arm, left flank, right flank) as the rule has them; bnd[k] = (first, last, arm of a JUDGED segment or 0, 0), the one
 * gather an end of a contact needs; the segments whose model sum has more than wave_pairs terms are listed in large[] (in any
 * order: every segment's sum is its own). */
__global__ void __launch_bounds__(ORIENT_THREADS) k_orient_segments(const int* __restrict__ first, const int* __restrict__ last, int n_seg, const int2* __restrict__ meta,
                                                                    int T, int window, long long wave_pairs, int4* __restrict__ geo, int4* __restrict__ bnd,
                                                                    int* __restrict__ large, int* __restrict__ ctl)
{
    const int k = blockIdx.x * ORIENT_THREADS + threadIdx.x;
    if (k >= n_seg) return;
    const int f = first[k], l = last[k];
    int err = 0;
    if (f < 0 || l < f || l >= T) err |= 1;
    if (k > 0 && f <= last[k - 1]) err |= 2;
    int4 g = make_int4(0, 0, 0, 0), b = make_int4(0, -1, 0, 0);
    if (!err) {
        const int2 mf = meta[f], ml = meta[l];
        if (mf.x != ml.x) err |= 4;
        else {
            const int n = l - f + 1;
            const bool ring = mf.y < 0;
            const int start = max(mf.x, 0), end = min(start + abs(mf.y), T);
            const int arm = ring ? 0 : min(n / 2, window);
            const int lf = ring ? 0 : min(window, f - start);
            const int rf = ring ? 0 : min(window, end - 1 - l);
            const int status = n < 2 ? 1 : ring ? 2 : lf + rf == 0 ? 3 : 0;
            g = make_int4(status, arm, lf, rf);
            b = make_int4(f, l, status == 0 ? arm : 0, 0);
            if (status == 0 && 2ll * arm * (long long)(lf + rf) > wave_pairs) large[atomicAdd(&ctl[ORIENT_CTL_LARGE], 1)] = k;
        }
    }
    geo[k] = g;
    bnd[k] = b;
    if (err) atomicOr(&ctl[ORIENT_CTL_ERR], err);
}

/* seg[r]: the segment position r lies in, -1: none -- one thread per position, a binary search over first[] (memory-safe whatever
 * the list holds: the host looks at the error word before anything reads seg) */
__global__ void __launch_bounds__(ORIENT_THREADS) k_orient_paint(const int* __restrict__ first, const int* __restrict__ last, int n_seg, int T, int* __restrict__ seg)
{
    const int r = blockIdx.x * ORIENT_THREADS + threadIdx.x;
    if (r >= T) return;
    int lo = 0, hi = n_seg; /* the segments in front of lo start at or before r */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    seg[r] = lo > 0 && last[lo - 1] >= r ? lo - 1 : -1;
}

/* The observed part: one pass over the contacts (row of contact k: crow[k]; column and count: cc[k]; row-major sorted), one 16-byte
 * record gather per end, seg[] at both positions and the 16-byte bounds of the segments found there.  Up to two atomics per
 * contact, on word 4 * segment + quadrant.
 *
 * COMBINE = false, the yardstick: one atomic per counted end.
 *
 * COMBINE = true: the lanes of a wave hold 64 consecutive contacts, mostly of one row, and the end of a contact that lies at its ROW
 * mostly falls into the same arm with the other end in the same flank: equal destinations of the row end next to each other are
 * summed inside the wave first (wave_runs and wave_run_sum, ig_kernels_wave.cuh) and only the head of a run issues the atomic.
 * The column end goes out as it is.  V: int where 64 counts cannot overflow one, else long long.
 *
 * The six classes of contact and the entries are summed in registers and reach memory once per workgroup.  A sharded handle takes
 * the rows i % world == rank: the ranks' quadrants and class sums add up. */
template <bool COMBINE, typename V>
__global__ void __launch_bounds__(ORIENT_THREADS) k_orient_observed(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z, const int4* __restrict__ rec,
                                                                    const int* __restrict__ seg, const int4* __restrict__ bnd, int window,
                                                                    unsigned long long* __restrict__ obs, unsigned long long* __restrict__ out_sc, int rank, int world)
{
    __shared__ unsigned long long sc[ORIENT_N_OBS];
    class_zero<ORIENT_N_OBS>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_unpl = 0, r_trans = 0, r_ring = 0, r_within = 0, r_counted = 0, r_uncounted = 0, r_entries = 0;
    const long long stride = (long long)gridDim.x * ORIENT_THREADS;
    const long long Zr = (Z + 63) & ~63LL; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * ORIENT_THREADS + threadIdx.x; k < Zr; k += stride) {
        int d_row = -1, d_col = -1; /* the words of the end at the contact's row and of the other, -1: not counted */
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
                    const int sa = seg[pa], sb = seg[pb];
                    if (sa >= 0 && sa == sb) r_within += cv;
                    else {
                        int d_lo = -1, d_hi = -1;
                        if (sa >= 0) { /* the lower end, for sa: pb in its right flank */
                            const int4 s = bnd[sa];
                            if (s.z > 0 && pb - s.y <= window) d_lo = pa < s.x + s.z ? 4 * sa + ORIENT_LR : pa > s.y - s.z ? 4 * sa + ORIENT_RR : -1;
                        }
                        if (sb >= 0) { /* the upper end, for sb: pa in its left flank */
                            const int4 s = bnd[sb];
                            if (s.z > 0 && s.x - pa <= window) d_hi = pb < s.x + s.z ? 4 * sb + ORIENT_LL : pb > s.y - s.z ? 4 * sb + ORIENT_RL : -1;
                        }
                        const int n_hit = (d_lo >= 0) + (d_hi >= 0);
                        if (n_hit) r_counted += cv;
                        else r_uncounted += cv;
                        r_entries += cv * (unsigned long long)n_hit;
                        const bool row_low = a.w < b.w;
                        d_row = row_low ? d_lo : d_hi;
                        d_col = row_low ? d_hi : d_lo;
                    }
                }
            }
        }
        if (d_col >= 0) atomicAdd(&obs[d_col], cv);
        if (!COMBINE) {
            if (d_row >= 0) atomicAdd(&obs[d_row], cv);
            continue;
        }
        V v = d_row >= 0 ? (V)(long long)cv : (V)0;
        const WaveRuns runs = wave_runs(d_row, lane);
        v = wave_run_sum<V>(runs, v, lane);
        if (runs.head && d_row >= 0 && v != 0) atomicAdd(&obs[d_row], (unsigned long long)(long long)v);
    }
    if (r_unpl) atomicAdd(&sc[ORIENT_UNPLACED], r_unpl);
    if (r_trans) atomicAdd(&sc[ORIENT_TRANS], r_trans);
    if (r_ring) atomicAdd(&sc[ORIENT_RING], r_ring);
    if (r_within) atomicAdd(&sc[ORIENT_WITHIN], r_within);
    if (r_counted) atomicAdd(&sc[ORIENT_COUNTED], r_counted);
    if (r_uncounted) atomicAdd(&sc[ORIENT_UNCOUNTED], r_uncounted);
    if (r_entries) atomicAdd(&sc[ORIENT_ENTRIES], r_entries);
    class_flush<ORIENT_N_OBS>(sc, out_sc);
}

/* The model part, no atomics on the arrays.  With q(i, k) = ig_quantize((double) ig_rippe(fabsf(ds_i - ds_k), p)) under the parameter
 * set the moves are scored under, a judged segment's 2 m (lf + rf) pairs (arm position, flank position) are evaluated and summed as
 * integers: expq[2 s] over the pairs of an arm with the flank on its own side (keep), expq[2 s + 1] over the others (flip).  The rows
 * of the segments that are not judged are written 0.
 *
 * G lanes share a segment.  G = 64, a wave with an integer wave reduction, launched over every segment: it leaves the segments with
 * more than wave_pairs terms alone.  G = ORIENT_THREADS, a workgroup (the waves' sums meet in LDS), launched over the list of those
 * segments k_orient_segments made (list = null: over every segment, as the wave form).  Integer sums: the result is the same either
 * way.  *maxq takes the largest |q| seen (the host's overflow guard). */
template <int G>
__global__ void __launch_bounds__(ORIENT_THREADS) k_orient_model(const float* __restrict__ ds, const int4* __restrict__ geo, const int4* __restrict__ bnd,
                                                                 const int* __restrict__ list, int n_items, long long wave_pairs, const Glob* __restrict__ g,
                                                                 unsigned long long* __restrict__ expq, unsigned long long* __restrict__ maxq)
{
    __shared__ unsigned long long part[2 * (ORIENT_THREADS / 64)];
    const int item = (int)(((long long)blockIdx.x * ORIENT_THREADS + threadIdx.x) / G);
    const int sub = threadIdx.x % G;
    const bool live = item < n_items; /* (uniform over the G lanes) */
    const int s = live ? (list ? list[item] : item) : -1;
    unsigned long long keep = 0, flip = 0, mx = 0;
    bool mine = false; /* this launch owns the segment's row */
    if (live) {
        const int4 ge = geo[s], b = bnd[s];
        const int m = b.z, lf = ge.z, rf = ge.w, nf = lf + rf; /* (b.z: 0 unless the segment is judged) */
        const long long terms = 2ll * m * (long long)nf;
        mine = list != nullptr || terms == 0 || terms <= wave_pairs;
        if (mine && terms > 0) {
            const ig_params p = g->par[0];
            for (long long t = sub; t < terms; t += G) {
                const int ia = (int)(t / nf), jf = (int)(t - (long long)ia * nf);
                const bool arm_left = ia < m, flank_left = jf < lf;
                const int pa = arm_left ? b.x + ia : b.y - 2 * m + 1 + ia;
                const int pf = flank_left ? b.x - lf + jf : b.y + 1 + (jf - lf);
                const long long q = ig_quantize((double)ig_rippe(fabsf(ds[pa] - ds[pf]), p, ig_tab()));
                if (arm_left == flank_left) keep += (unsigned long long)q;
                else flip += (unsigned long long)q;
                const unsigned long long aq = (unsigned long long)(q < 0 ? -q : q);
                mx = aq > mx ? aq : mx;
            }
        }
    }
    /* (one loop for the maximum and the sums: their shuffles interleave, as in k_junc_model) */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
        keep += __shfl_xor(keep, d, 64);
        flip += __shfl_xor(flip, d, 64);
    }
    if (G == 64) {
        if (mine && sub == 0) {
            expq[2 * (size_t)s] = keep;
            expq[2 * (size_t)s + 1] = flip;
        }
    } else {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            part[2 * wave] = keep;
            part[2 * wave + 1] = flip;
        }
        __syncthreads();
        if (mine && threadIdx.x == 0) {
            unsigned long long a = 0, c = 0;
            for (int w = 0; w < ORIENT_THREADS / 64; w++) {
                a += part[2 * w];
                c += part[2 * w + 1];
            }
            expq[2 * (size_t)s] = a;
            expq[2 * (size_t)s + 1] = c;
        }
    }
    if ((threadIdx.x & 63) == 0) raise_max(maxq, mx);
}
