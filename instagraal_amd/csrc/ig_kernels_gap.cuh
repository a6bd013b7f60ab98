/* ig_kernels_gap.cuh -- gap support: the distance the contacts put across each join of the current genome.  The caller lists
 * junctions j (between the positions j - 1 and j of the genome order, each internal to one placed contig) and K gaps g_0 = 0 < g_1 <
 * ... in kb; for every junction the contacts that span it inside a window of w positions are summed next to the two halves of a
 * Poisson log-likelihood under every gap: with E_k = ig_rippe(s + g_k, p), s = fabsf(ds_i - ds_m) the separation of a pair,
 * expected_q[j][k] = the sum over the pairs (i, m), i < j <= m, m - i <= w, of ig_quantize(E_k) and log_q[j][k] = the sum over the
 * spanning contacts of cnt * ig_quantize(ig_log10(E_k)).  The rule is stated once, in instagraal_amd/gap_support.py; the kernels here
 * reproduce it byte for byte.
 *
 * Integer sums throughout (unsigned wrap-around adds): the result does not depend on threads, waves, workgroups or the order of the
 * atomics.  The records, ds, meta and the order are the genome view's (ig_kernels_genome.cuh).
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define GAP_THREADS 256
#define GAP_MAX_WINDOW 256 /* this report's own: a junction costs K w (w + 1) / 2 model values */
#define GAP_MIN_GAPS 2
#define GAP_MAX_GAPS 64
#define GAP_NS 8 /* scalars: the order of ig_gap_support's scalars[8] */
#define GAP_UNPLACED 0
#define GAP_TRANS 1
#define GAP_RING 2
#define GAP_COUNTED 3
#define GAP_UNCOUNTED 4
#define GAP_CONTRIB 5
#define GAP_N_OBS 6     /* (the words the observed pass owns) */
#define GAP_JUDGED 6    /* (counted on the host from the status) */
#define GAP_PLACED 7    /* (the host's T) */
#define GAP_DEV_MAXE 6  /* on the device that word holds the largest |quantised model value| the model pass saw */
#define GAP_DEV_MAXL 7  /* ... and that one the largest |quantised log10 of a model value| the observed pass saw */
#define GAP_WAVE_TERMS 8192 /* junctions with pairs * K beyond this: a workgroup per junction in the model pass, else a wave */
/* the words of GapBuf.ctl */
#define GAP_CTL_ERR 0   /* k_gap_junctions: the list is malformed (bit 0 range, 1 order, 2 a contig boundary) */
#define GAP_CTL_LARGE 1 /* ... junctions listed for the workgroup form of the model pass */

/* One thread per listed junction k: the list is checked -- in range, strictly ascending (against the junction in front), both sides
 * in one contig by meta -- and a malformed one sets the error word: the host fails loudly and nothing is written out of bounds.
 * status[k] = 0 judged, 2 on a ring; geo[k] = (the BIN at position j: the host turns it into the canonical id of its contig, left,
 * right, 0) as the rule has them; pairs[k] by the closed form of junction_profile.pairs_closed_form; the judged junctions whose
 * model sum has more than wave_terms terms are listed in large[] (in any order: every junction's sums are its own). */
__global__ void __launch_bounds__(GAP_THREADS) k_gap_junctions(const int* __restrict__ junc, int n_junc, const int2* __restrict__ meta, const int* __restrict__ order,
                                                               const SubTab* __restrict__ sub, int M, int T, int window, int n_gaps, long long wave_terms,
                                                               int* __restrict__ status, int4* __restrict__ geo, unsigned long long* __restrict__ pairs,
                                                               int* __restrict__ large, int* __restrict__ ctl)
{
    const int k = blockIdx.x * GAP_THREADS + threadIdx.x;
    if (k >= n_junc) return;
    const int j = junc[k];
    int err = 0;
    if (j < 1 || j >= T) err |= 1;
    if (k > 0 && j <= junc[k - 1]) err |= 2;
    int st = 0;
    int4 g = make_int4(-1, 0, 0, 0);
    long long np = 0;
    if (!err) {
        const int2 ma = meta[j - 1], mb = meta[j];
        if (ma.x != mb.x) err |= 4;
        else {
            const bool ring = mb.y < 0;
            const int start = max(mb.x, 0), end = min(start + abs(mb.y), T);
            const int s = order[j];
            g.x = (unsigned)s < (unsigned)M ? sub[s].parent : -1;
            if (ring) st = 2;
            else {
                const long long w = window, a = min(window, j - start), b = end - j; /* F(x) = sum_{v = 1 .. x} min(b, v) */
                const long long x1 = w - a;
                const long long Fw = w <= b ? w * (w + 1) / 2 : b * (b + 1) / 2 + (w - b) * b;
                const long long Fx = x1 <= b ? x1 * (x1 + 1) / 2 : b * (b + 1) / 2 + (x1 - b) * b;
                np = Fw - Fx;
                g.y = (int)a;
                g.z = (int)min(w, b);
                if (np * (long long)n_gaps > wave_terms) large[atomicAdd(&ctl[GAP_CTL_LARGE], 1)] = k;
            }
        }
    }
    status[k] = st;
    geo[k] = g;
    pairs[k] = (unsigned long long)np;
    if (err) atomicOr(&ctl[GAP_CTL_ERR], err);
}

/* nj[r]: the number of listed junctions <= r -- one thread per position, a binary search over the list (memory-safe whatever the
 * list holds: the host looks at the error word before anything reads nj).  A contact at pa < pb then spans exactly the list indices
 * nj[pa] .. nj[pb] - 1. */
__global__ void __launch_bounds__(GAP_THREADS) k_gap_paint(const int* __restrict__ junc, int n_junc, int T, int* __restrict__ nj)
{
    const int r = blockIdx.x * GAP_THREADS + threadIdx.x;
    if (r >= T) return;
    int lo = 0, hi = n_junc; /* the junctions in front of lo are <= r */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (junc[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    nj[r] = lo;
}

/* The observed part: one pass over the contacts (row of contact k: crow[k]; column and count: cc[k]; row-major sorted), one 16-byte
 * record gather per end, nj[] at both positions.  The K values ig_quantize(ig_log10(E_k)) depend on the contact only: each is
 * evaluated once per contact (the gaps in LDS) and added, times the count, to every junction the contact spans -- a listed junction
 * between two positions of one linear contig is judged --, the count itself to observed[].  One 64-bit no-return atomic per word.
 *
 * The five classes of contact and the contributions are summed in registers and reach memory once per workgroup, the largest
 * |quantised log| once per wave.  A sharded handle takes the rows i % world == rank: the ranks' observed, log_q and class sums add
 * up. */
__global__ void __launch_bounds__(GAP_THREADS) k_gap_observed(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z, const int4* __restrict__ rec,
                                                              const int* __restrict__ nj, const float* __restrict__ gaps, int n_gaps, int window,
                                                              const Glob* __restrict__ g, unsigned long long* __restrict__ obs,
                                                              unsigned long long* __restrict__ logq, unsigned long long* __restrict__ out_sc, int rank, int world)
{
    __shared__ unsigned long long sc[GAP_N_OBS];
    __shared__ float sg[GAP_MAX_GAPS];
    if (threadIdx.x < GAP_MAX_GAPS) sg[threadIdx.x] = threadIdx.x < n_gaps ? gaps[threadIdx.x] : 0.0f;
    class_zero<GAP_N_OBS>(sc); /* (its barrier covers the gaps too) */
    const ig_params p = g->par[0];
    unsigned long long r_unpl = 0, r_trans = 0, r_ring = 0, r_counted = 0, r_uncounted = 0, r_contrib = 0, mx = 0;
    const long long stride = (long long)gridDim.x * GAP_THREADS;
    for (long long k = (long long)blockIdx.x * GAP_THREADS + threadIdx.x; k < Z; k += stride) {
        const int i = crow[k];
        if (!contact_is_mine(i, rank, world)) continue;
        const int2 e = cc[k];
        const int4 a = rec[i], b = rec[e.x];
        const unsigned long long cv = (unsigned long long)(long long)e.y;
        const GenomePair cls = genome_pair_class(a, b);
        if (cls == PAIR_UNPLACED) r_unpl += cv;
        else if (cls == PAIR_TRANS) r_trans += cv;
        else if (cls == PAIR_RING) r_ring += cv;
        else {
            const int pa = min(a.w, b.w), pb = max(a.w, b.w);
            const int lo = nj[pa], hi = pb - pa <= window ? nj[pb] : lo;
            if (hi <= lo) {
                r_uncounted += cv;
                continue;
            }
            r_counted += cv;
            r_contrib += (unsigned long long)(hi - lo);
            for (int jj = lo; jj < hi; jj++) atomicAdd(&obs[jj], cv);
            const float s = fabsf(__int_as_float(a.x) - __int_as_float(b.x));
            for (int q = 0; q < n_gaps; q++) {
                const long long lq = ig_quantize(ig_log10((double)ig_rippe(s + sg[q], p, ig_tab()), ig_tab()));
                const unsigned long long al = (unsigned long long)(lq < 0 ? -lq : lq);
                mx = al > mx ? al : mx;
                const unsigned long long v = cv * (unsigned long long)lq;
                for (int jj = lo; jj < hi; jj++) atomicAdd(&logq[(size_t)jj * n_gaps + q], v);
            }
        }
    }
    if (r_unpl) atomicAdd(&sc[GAP_UNPLACED], r_unpl);
    if (r_trans) atomicAdd(&sc[GAP_TRANS], r_trans);
    if (r_ring) atomicAdd(&sc[GAP_RING], r_ring);
    if (r_counted) atomicAdd(&sc[GAP_COUNTED], r_counted);
    if (r_uncounted) atomicAdd(&sc[GAP_UNCOUNTED], r_uncounted);
    if (r_contrib) atomicAdd(&sc[GAP_CONTRIB], r_contrib);
    mx = wave_max_u64(mx);
    if ((threadIdx.x & 63) == 0) raise_max(&out_sc[GAP_DEV_MAXL], mx);
    class_flush<GAP_N_OBS>(sc, out_sc);
}

/* The model part, no atomics on the arrays.  A judged junction j with `left` positions in front and `right` behind has the pairs
 * (j - 1 - u, j + v), u < left, v < right, u + v + 1 <= w; the ds of those left + right <= 2 w positions are staged in LDS once,
 * then for every gap k the lanes that share the junction run over the left x right rectangle, evaluate
 * ig_quantize((double) ig_rippe(fabsf(ds_i - ds_m) + g_k, p)) where the pair is in the window and sum as integers:
 * expq[j * K + k].  The rows of the junctions that are not judged are written 0.
 *
 * G lanes share a junction.  G = 64, a wave with an integer wave reduction, launched over every junction: it leaves the junctions
 * with more than wave_terms terms alone.  G = GAP_THREADS, a workgroup (the waves' sums meet in LDS), launched over the list of
 * those junctions k_gap_junctions made (list = null: over every junction, as the wave form).  Integer sums: the result is the same
 * either way.  *maxq takes the largest |q| seen (the host's overflow guard). */
template <int G>
__global__ void __launch_bounds__(GAP_THREADS) k_gap_model(const float* __restrict__ ds, const int* __restrict__ junc, const int* __restrict__ status,
                                                           const int4* __restrict__ geo, const unsigned long long* __restrict__ pairs,
                                                           const int* __restrict__ list, int n_items, const float* __restrict__ gaps, int n_gaps, int window,
                                                           long long wave_terms, const Glob* __restrict__ g, unsigned long long* __restrict__ expq,
                                                           unsigned long long* __restrict__ maxq)
{
    constexpr int GROUPS = GAP_THREADS / G; /* junctions per workgroup */
    __shared__ float sds[GROUPS][2 * GAP_MAX_WINDOW];
    __shared__ float sg[GAP_MAX_GAPS];
    __shared__ unsigned long long part[GAP_THREADS / 64][GAP_MAX_GAPS];
    const int grp = threadIdx.x / G, sub = threadIdx.x % G;
    const int item = blockIdx.x * GROUPS + grp;
    const bool live = item < n_items; /* (uniform over the G lanes) */
    const int s = live ? (list ? list[item] : item) : -1;
    int left = 0, right = 0;
    bool mine = false; /* this launch owns the junction's row */
    if (threadIdx.x < GAP_MAX_GAPS) sg[threadIdx.x] = threadIdx.x < n_gaps ? gaps[threadIdx.x] : 0.0f;
    if (live) {
        const int4 ge = geo[s];
        const long long terms = status[s] == 0 ? (long long)pairs[s] * n_gaps : 0;
        mine = list != nullptr || terms == 0 || terms <= wave_terms;
        if (mine && terms > 0) {
            left = min(ge.y, GAP_MAX_WINDOW); /* (the rule's left, right <= w <= GAP_MAX_WINDOW: the clamp keeps LDS safe whatever geo holds) */
            right = min(ge.z, GAP_MAX_WINDOW);
            const int j = junc[s];
            for (int o = sub; o < left + right; o += G) sds[grp][o] = ds[j - left + o]; /* position j - left + o: j - 1 - u sits at left - 1 - u, j + v at left + v */
        }
    }
    __syncthreads();
    const ig_params p = g->par[0];
    const int cells = left * right; /* (<= 2^16) */
    unsigned long long mx = 0;
    for (int q = 0; q < n_gaps; q++) {
        unsigned long long acc = 0;
        const float gq = sg[q];
        for (int t = sub; t < cells; t += G) {
            const int u = t / right, v = t - u * right;
            if (u + v + 1 > window) continue;
            const long long e = ig_quantize((double)ig_rippe(fabsf(sds[grp][left - 1 - u] - sds[grp][left + v]) + gq, p, ig_tab()));
            acc += (unsigned long long)e;
            const unsigned long long ae = (unsigned long long)(e < 0 ? -e : e);
            mx = ae > mx ? ae : mx;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d, 64); /* (inline: through wave_sum_u64 the loop over the gaps is scheduled another way) */
        if (G == 64) {
            if (mine && sub == 0) expq[(size_t)s * n_gaps + q] = acc;
        } else if ((threadIdx.x & 63) == 0)
            part[threadIdx.x >> 6][q] = acc;
    }
    if (G != 64) {
        __syncthreads();
        if (mine && threadIdx.x < n_gaps) {
            unsigned long long a = 0;
            for (int w = 0; w < GAP_THREADS / 64; w++) a += part[w][threadIdx.x];
            expq[(size_t)s * n_gaps + threadIdx.x] = a;
        }
    }
    mx = wave_max_u64(mx);
    if ((threadIdx.x & 63) == 0) raise_max(maxq, mx);
}
