/* ig_kernels_law.cuh -- the distance law P(s) of the current genome as the data shows it: per bin of genomic separation the contacts
 * observed and the sub-fragment pairs that could have had one.  The rule is stated once, in instagraal_amd/distance_law.py; the
 * kernels here reproduce it entry for entry (64-bit integer sums: exact, independent of the grid and of the order of the atomics).
 *
 * A pair of sub-fragments of one PLACED contig (every bin active: the contact map's rule, k_map_pixels) that is not a ring has the
 * separation s = fabsf(dist_i - dist_j) -- what the exact cis term feeds the model (eval_q) -- and the bin b with
 * edges[b] <= s < edges[b + 1].  Pairs on a ring have two separations and are counted apart; so are trans pairs, contacts with an
 * end that is not placed, and separations outside the edges.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define LAW_THREADS 256
#define LAW_MAX_EDGES 4097
#define LAW_MAX_BINS (LAW_MAX_EDGES - 1)
#define LAW_NS 8 /* scalars: the order of ig_distance_law's scalars[8] */
#define LAW_OOR_OBS 0
#define LAW_OOR_PAIRS 1
#define LAW_TRANS_OBS 2
#define LAW_TRANS_PAIRS 3 /* (from T and LAW_PLACED_PAIRS on the host) */
#define LAW_RING_OBS 4
#define LAW_RING_PAIRS 5
#define LAW_UNPLACED_OBS 6
#define LAW_PLACED_PAIRS 7

/* LDS of both passes (dynamic: a law of 100 bins leaves the occupancy alone): the workgroup's histogram, its scalars, the edges */
__host__ __device__ inline size_t law_lds_bytes(int n_edges) { return (size_t)(n_edges - 1 + LAW_NS) * 8 + (size_t)n_edges * 4; }

/* edges[b] <= s < edges[b + 1]  <=>  b = (number of edges <= s) - 1: comparisons only */
__device__ __forceinline__ int law_upper_bound(const float* e, int n_edges, float s)
{
    int lo = 0, hi = n_edges;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void law_lds_setup(const float* __restrict__ edges, int n_edges, unsigned long long*& hist, unsigned long long*& sc, float*& e)
{
    extern __shared__ unsigned long long law_lds[];
    const int nb = n_edges - 1;
    hist = law_lds;
    sc = hist + nb;
    e = (float*)(sc + LAW_NS);
    for (int i = threadIdx.x; i < n_edges; i += blockDim.x) e[i] = edges[i];
    for (int i = threadIdx.x; i < nb + LAW_NS; i += blockDim.x) hist[i] = 0ull;
    __syncthreads();
}

/* the workgroup's scalars and histogram to memory: native 64-bit atomics, non-zero entries only (class_flush's barrier stands in
 * front of both) */
__device__ __forceinline__ void law_lds_flush(const unsigned long long* hist, const unsigned long long* sc, int nb, unsigned long long* __restrict__ out_hist,
                                              unsigned long long* __restrict__ out_sc)
{
    class_flush<LAW_NS>(sc, out_sc);
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const unsigned long long v = hist[i];
        if (v) atomicAdd(&out_hist[i], v);
    }
}

/* The observed part: one pass over the contacts (row of contact k: crow[k]; column and count: cc[k]).
 *
 * PRIV = false, the yardstick: one global atomic per contact.
 *
 * PRIV = true: every workgroup keeps its own histogram in LDS (64-bit LDS adds) and flushes it once.  The scalars -- most contacts
 * of a scaffold in progress are trans: one address for the whole wave -- are summed in registers and reach LDS once per thread.
 * A sharded handle takes the rows i % world == rank: the ranks' results add up. */
template <bool PRIV>
__global__ void __launch_bounds__(LAW_THREADS) k_law_observed(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                              const int4* __restrict__ rec, const float* __restrict__ edges, int n_edges,
                                                              unsigned long long* __restrict__ out_hist, unsigned long long* __restrict__ out_sc,
                                                              int rank, int world)
{
    unsigned long long *hist, *sc;
    float* e;
    law_lds_setup(edges, n_edges, hist, sc, e);
    const int nb = n_edges - 1;
    unsigned long long r_oor = 0, r_trans = 0, r_ring = 0, r_unpl = 0;
    const long long stride = (long long)gridDim.x * LAW_THREADS;
    for (long long k = (long long)blockIdx.x * LAW_THREADS + threadIdx.x; k < Z; k += stride) {
        const int i = crow[k];
        if (!contact_is_mine(i, rank, world)) continue;
        const int2 c = cc[k];
        const int4 a = rec[i], b = rec[c.x];
        const unsigned long long v = (unsigned long long)(long long)c.y;
        const GenomePair cls = genome_pair_class(a, b);
        int which; /* >= 0: a bin, else -1 - scalar */
        if (cls == PAIR_UNPLACED) which = -1 - LAW_UNPLACED_OBS;
        else if (cls == PAIR_TRANS) which = -1 - LAW_TRANS_OBS;
        else if (cls == PAIR_RING) which = -1 - LAW_RING_OBS;
        else {
            const float s = fabsf(__int_as_float(a.x) - __int_as_float(b.x));
            const int ub = law_upper_bound(e, n_edges, s);
            which = (ub == 0 || ub == n_edges) ? -1 - LAW_OOR_OBS : ub - 1;
        }
        if (!PRIV) {
            atomicAdd(which >= 0 ? &out_hist[which] : &out_sc[-1 - which], v);
            continue;
        }
        if (which >= 0) atomicAdd(&hist[which], v);
        else if (which == -1 - LAW_TRANS_OBS) r_trans += v;
        else if (which == -1 - LAW_UNPLACED_OBS) r_unpl += v;
        else if (which == -1 - LAW_RING_OBS) r_ring += v;
        else r_oor += v;
    }
    if (!PRIV) return;
    if (r_oor) atomicAdd(&sc[LAW_OOR_OBS], r_oor);
    if (r_trans) atomicAdd(&sc[LAW_TRANS_OBS], r_trans);
    if (r_ring) atomicAdd(&sc[LAW_RING_OBS], r_ring);
    if (r_unpl) atomicAdd(&sc[LAW_UNPLACED_OBS], r_unpl);
    law_lds_flush(hist, sc, nb, out_hist, out_sc);
}

/* The pairs part: one thread per placed sub-fragment i at position r of the genome order, for the pairs (i, j) with j BEHIND it in
 * its contig (every unordered pair once).
 *
 * BRUTE = false.  dist does not decrease with the rank inside a contig (the tables' definition, k_fill_tables) and the f32
 * subtraction is monotone in dist_j, so s(j) = fabsf(dist_j - dist_i) does not decrease in j: the j behind i fall into the bins in
 * runs.  The thread finds the bin of the first j of a run by a binary search over the edges, the end of the run -- the first j whose
 * s reaches the bin's upper edge -- by a galloping search over the contig's slice of ds, and adds the run's length to the bin: work
 * per thread ~ (bins that hold a pair of it) x log, whatever the contig's length.  A thread that sees dist DEcrease at its own
 * position raises *nonmono; the host then discards the pass and runs the other form, which assumes nothing.
 *
 * BRUTE = true: every j, one by one (equal bins in a row are added once). */
template <bool BRUTE>
__global__ void __launch_bounds__(LAW_THREADS) k_law_pairs(const float* __restrict__ ds, const int2* __restrict__ meta, int T,
                                                           const float* __restrict__ edges, int n_edges, unsigned long long* __restrict__ out_hist,
                                                           unsigned long long* __restrict__ out_sc, int* __restrict__ nonmono)
{
    unsigned long long *hist, *sc;
    float* e;
    law_lds_setup(edges, n_edges, hist, sc, e);
    const int nb = n_edges - 1;
    const int r = blockIdx.x * LAW_THREADS + threadIdx.x;
    if (r < T) {
        const int2 m = meta[r];
        const bool ring = m.y < 0;
        const int start = max(m.x, 0);
        const int end = min(start + (ring ? -m.y : m.y), T);
        const unsigned long long behind = end - 1 > r ? (unsigned long long)(end - 1 - r) : 0ull;
        unsigned long long oor = 0;
        if (behind && !ring) {
            const float di = ds[r];
            if (BRUTE) {
                int cur = -2, run = 0; /* the bin of the run in hand (-1: out of range) */
                for (int j = r + 1; j < end; j++) {
                    const int ub = law_upper_bound(e, n_edges, fabsf(ds[j] - di));
                    const int b = (ub == 0 || ub == n_edges) ? -1 : ub - 1;
                    if (b != cur) {
                        if (run && cur >= 0) atomicAdd(&hist[cur], (unsigned long long)run);
                        else oor += run;
                        cur = b;
                        run = 0;
                    }
                    run++;
                }
                if (run && cur >= 0) atomicAdd(&hist[cur], (unsigned long long)run);
                else oor += run;
            } else {
                if (ds[r + 1] < di) atomicOr(nonmono, 1);
                int j = r + 1;
                while (j < end) {
                    const int ub = law_upper_bound(e, n_edges, fabsf(ds[j] - di));
                    if (ub == n_edges) { /* at or beyond the last edge, and so is everything behind */
                        oor += (unsigned long long)(end - j);
                        break;
                    }
                    const float limit = e[ub]; /* the first edge above s(j): the run ends at the first j' with s(j') >= limit */
                    int lo = j, hi = j + 1, step = 1;
                    while (hi < end && fabsf(ds[hi] - di) < limit) {
                        lo = hi;
                        step <<= 1;
                        hi = (end - lo > step) ? lo + step : end;
                    }
                    while (lo + 1 < hi) { /* s(lo) < limit; hi == end or s(hi) >= limit */
                        const int mid = lo + ((hi - lo) >> 1);
                        if (fabsf(ds[mid] - di) < limit) lo = mid;
                        else hi = mid;
                    }
                    const unsigned long long n = (unsigned long long)(hi - j);
                    if (ub == 0) oor += n;
                    else atomicAdd(&hist[ub - 1], n);
                    j = hi;
                }
            }
        }
        if (behind) atomicAdd(&sc[LAW_PLACED_PAIRS], behind);
        if (behind && ring) atomicAdd(&sc[LAW_RING_PAIRS], behind);
        if (oor) atomicAdd(&sc[LAW_OOR_PAIRS], oor);
    }
    law_lds_flush(hist, sc, nb, out_hist, out_sc);
}
