/* ig_kernels_bal.cuh -- balancing the contact map of the current genome: one weight per UNIT (level 0: the positions of the genome
 * order; 1: the placed bins along it; 2: the pixels of the contact map) by iterative correction.  The rule is stated once, in
 * instagraal_amd/balance.py; the passes here reproduce its arrays byte for byte.
 *
 * The rows: k_bal_emit is the counting sort of k_place_emit with two emissions per kept contact, entry = (row: the unit of one end,
 * word: the unit of the other end << 32 | count); the rows are sorted and the equal columns summed by the row builder
 * (ig_kernels_rows.cuh).  The units are the lift's keys (k_lift_heads, k_lift_keys).
 * The iteration: k_bal_marginals, the hot kernel, a sparse matrix-vector product in the rule's ORDERED SUM -- lane l of a wave is
 * accumulator l, takes the row's entries l, l + 64, ... in that order, and the 64 accumulators are combined by the tree
 * a[l] += a[l + h], h = 32 .. 1, six __shfl_down.  Doubles, + * / only, no atomics on them, and no fma where the rule has * then +
 * (the translation unit is compiled with -ffp-contract=off): the bytes are numpy's.  The steps over the units (k_bal_mean,
 * k_bal_update, k_bal_var) stay on the device; wave 0 of one workgroup does the two ordered sums over all units.  A done flag
 * (BalCtl) turns every kernel enqueued behind the last iteration of the rule into a no-op, so the host may enqueue iterations in
 * groups and still get the rule's b, n_iters and variance.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define BAL_THREADS 256
#define BAL_NS 5 /* the scalars the passes over the contacts own: the order of ig_balance_build's scalars[0..4] */
#define BAL_UNPLACED_OBS 0
#define BAL_WITHIN_OBS 1
#define BAL_BAND_OBS 2
#define BAL_KEPT_OBS 3
#define BAL_ENTRIES 4
#define BAL_PACK_LANES 16 /* the packed form: a row of at most this many entries is served by this many lanes, four rows per wave */

/* what the loop's kernels share on the device */
struct BalCtl {
    double mean, k; /* of the iteration in flight: vec_sum(marg) / k, and k = the units with marg != 0 */
    int done;       /* the rule has stopped: every kernel of the loop behind it does nothing */
    int converged, n_iters, pad;
};

/* One pass over the contacts (row of contact k: crow[k]; column and count: cc[k]), twice, shaped like k_place_emit.
 * SCATTER = false: a contact is classified by the first class it fits (an end not placed, both ends in one unit, inside the ignored
 * band |u - v| < ignore_diags, kept); a kept contact counts for the rows of both units and for their totals.  The class sums and the
 * entries are summed in registers and reach memory once per workgroup.
 * SCATTER = true: the counters have become cursors; each of the two emissions takes the next slot of its row and writes (the unit of
 * the other end, count) there.  n_ent: the entries the first pass counted -- nothing is written beyond them. */
template <bool SCATTER>
__global__ void __launch_bounds__(BAL_THREADS) k_bal_emit(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                          const int* __restrict__ key, int U, int ignore_diags,
                                                          unsigned long long* __restrict__ counter, unsigned long long* __restrict__ total,
                                                          unsigned long long* __restrict__ ent, unsigned long long n_ent,
                                                          unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[BAL_NS];
    if (!SCATTER) class_zero<BAL_NS>(sc);
    unsigned long long r_unpl = 0, r_within = 0, r_band = 0, r_kept = 0, r_ent = 0;
    const long long stride = (long long)gridDim.x * BAL_THREADS;
    for (long long k = (long long)blockIdx.x * BAL_THREADS + threadIdx.x; k < Z; k += stride) {
        const int i = crow[k];
        const int2 e = cc[k];
        const int a = key[i], b = key[e.x];
        const unsigned long long cv = (unsigned long long)(long long)e.y;
        if (a < 0 || b < 0 || a >= U || b >= U) r_unpl += cv;
        else if (a == b) r_within += cv;
        else if (abs(a - b) < ignore_diags) r_band += cv;
        else if (!SCATTER) {
            r_kept += cv;
            r_ent += 2ull;
            atomicAdd(&counter[a], 1ull);
            atomicAdd(&counter[b], 1ull);
            atomicAdd(&total[a], cv);
            atomicAdd(&total[b], cv);
        } else {
            const unsigned long long sa = atomicAdd(&counter[a], 1ull), sb = atomicAdd(&counter[b], 1ull);
            if (sa < n_ent) ent[sa] = lift_pack(b, e.y);
            if (sb < n_ent) ent[sb] = lift_pack(a, e.y);
        }
    }
    if (SCATTER) return;
    if (r_unpl) atomicAdd(&sc[BAL_UNPLACED_OBS], r_unpl);
    if (r_within) atomicAdd(&sc[BAL_WITHIN_OBS], r_within);
    if (r_band) atomicAdd(&sc[BAL_BAND_OBS], r_band);
    if (r_kept) atomicAdd(&sc[BAL_KEPT_OBS], r_kept);
    if (r_ent) atomicAdd(&sc[BAL_ENTRIES], r_ent);
    class_flush<BAL_NS>(sc, out_sc);
}

/* the rows and what a term of the sum is made of.  RAW: the term is values[e] (ig_debug_lane_sums: the ordered sum over caller data);
 * otherwise float64(cnt[e]) * b[col[e]], one rounding (cnt < 2^53: the build's refusal) */
struct BalRows {
    const unsigned long long* rowptr; /* [n_rows + 1] */
    const int* col;
    const unsigned long long* cnt;
    const double* b;
    const double* values;
};

template <bool RAW>
__device__ __forceinline__ double bal_term(const BalRows& r, long long e)
{
    return RAW ? r.values[e] : (double)r.cnt[e] * r.b[r.col[e]];
}

/* The ordered sum of the entries [e0, e1) by the G lanes of a group, lane: 0 .. G - 1 -> lane 0 holds the sum.  G = 64 is the rule as
 * it is written.  G < 64 serves a row of at most G entries only: the accumulators G .. 63 of the rule stay +0.0 there, the tree's
 * steps h >= G add +0.0 to accumulators that are not -0.0 (they started from +0.0), which changes nothing: the same bytes.
 * Lane l + h of a step is right as long as l + h < 2 h, which is all lane 0's chain ever reads. */
template <int G, bool RAW>
__device__ __forceinline__ double bal_lane_sum(const BalRows& r, long long e0, long long e1, int lane)
{
    double acc = 0.0;
    for (long long e = e0 + lane; e < e1; e += G) acc += bal_term<RAW>(r, e);
#pragma unroll
    for (int h = G / 2; h >= 1; h >>= 1) acc += __shfl_down(acc, h, G);
    return acc;
}

/* a row's entries, clamped to the entries there are (an inconsistent rowptr reads nothing out of bounds) */
__device__ __forceinline__ void bal_row(const BalRows& r, long long row, long long n_ent, long long* e0, long long* e1)
{
    *e1 = (long long)min(r.rowptr[row + 1], (unsigned long long)n_ent);
    *e0 = min((long long)r.rowptr[row], *e1);
}

/* out[row] = lane_sum(row) (RAW), or lane_sum(row) * b[row]: the marginals.  done (may be null): the loop's flag.
 * PACKED = false, the yardstick: a wave per row.
 * PACKED = true: a wave per four consecutive rows; where all four have at most BAL_PACK_LANES entries, sixteen lanes serve each, all at
 * once; otherwise the wave takes the four one after the other as the yardstick does.  Whole waves branch together. */
template <bool RAW, bool PACKED>
__global__ void __launch_bounds__(BAL_THREADS) k_bal_marginals(BalRows r, long long n_rows, long long n_ent, const int* __restrict__ done,
                                                               double* __restrict__ out)
{
    if (done && *done) return;
    const long long wave = ((long long)blockIdx.x * BAL_THREADS + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (!PACKED) {
        if (wave >= n_rows) return;
        long long e0, e1;
        bal_row(r, wave, n_ent, &e0, &e1);
        const double s = bal_lane_sum<64, RAW>(r, e0, e1, lane);
        if (lane == 0) out[wave] = RAW ? s : s * r.b[wave];
        return;
    }
    constexpr int per_wave = 64 / BAL_PACK_LANES;
    const long long first = wave * per_wave;
    if (first >= n_rows) return;
    const long long mine = first + lane / BAL_PACK_LANES;
    long long e0 = 0, e1 = 0;
    if (mine < n_rows) bal_row(r, mine, n_ent, &e0, &e1);
    if (__all(e1 - e0 <= BAL_PACK_LANES)) {
        const int sub = lane % BAL_PACK_LANES;
        const double s = bal_lane_sum<BAL_PACK_LANES, RAW>(r, e0, e1, sub);
        if (sub == 0 && mine < n_rows) out[mine] = RAW ? s : s * r.b[mine];
        return;
    }
    for (int j = 0; j < per_wave && first + j < n_rows; j++) {
        bal_row(r, first + j, n_ent, &e0, &e1);
        const double s = bal_lane_sum<64, RAW>(r, e0, e1, lane);
        if (lane == 0) out[first + j] = RAW ? s : s * r.b[first + j];
    }
}

/* vec_sum by wave 0 of the workgroup: the ordered sum over one row of all of x -> lane 0 holds it.  A lane's additions are a chain,
 * its loads are not: eight of them are in flight before the first is added, in the rule's order (a single wave has nothing else to
 * hide the memory's latency behind) */
__device__ __forceinline__ double bal_vec_sum(const double* __restrict__ x, long long n, int lane)
{
    double acc = 0.0;
    long long i = lane;
    for (; i + 7 * 64 < n; i += 8 * 64) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = x[i + k * 64];
#pragma unroll
        for (int k = 0; k < 8; k++) acc += v[k];
    }
    for (; i < n; i += 64) acc += x[i];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) acc += __shfl_down(acc, h, 64);
    return acc;
}

/* one workgroup: k = the units with marg != 0 (every thread counts; integers), mean = vec_sum(marg) / k (wave 0).  k == 0: the rule
 * stops here, not converged, n_iters as reached. */
__global__ void __launch_bounds__(BAL_THREADS) k_bal_mean(const double* __restrict__ marg, long long n, BalCtl* __restrict__ ctl)
{
    __shared__ unsigned long long k_sh;
    const int done = ctl->done;
    if (threadIdx.x == 0) k_sh = 0ull;
    __syncthreads(); /* (every thread has read the flag before one of them may set it) */
    if (done) return;
    unsigned long long k = 0;
    for (long long i = threadIdx.x; i < n; i += BAL_THREADS) k += marg[i] != 0.0 ? 1ull : 0ull;
    if (k) atomicAdd(&k_sh, k);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const double s = bal_vec_sum(marg, n, threadIdx.x);
    if (threadIdx.x != 0) return;
    if (k_sh == 0ull) {
        ctl->done = 1;
        return;
    }
    ctl->k = (double)k_sh;
    ctl->mean = s / (double)k_sh;
}

/* m = marg / mean where marg != 0, else 1;  b = b / m;  dd = (m - 1)^2 where marg != 0, else 0 */
__global__ void __launch_bounds__(BAL_THREADS) k_bal_update(const double* __restrict__ marg, long long n, const BalCtl* __restrict__ ctl,
                                                            double* __restrict__ b, double* __restrict__ dd)
{
    if (ctl->done) return;
    const long long i = (long long)blockIdx.x * BAL_THREADS + threadIdx.x;
    if (i >= n) return;
    const double mg = marg[i], mean = ctl->mean;
    const bool nz = mg != 0.0;
    const double m = nz ? mg / mean : 1.0;
    b[i] = b[i] / m;
    const double d = nz ? m - 1.0 : 0.0;
    dd[i] = d * d;
}

/* wave 0 of one workgroup: var = vec_sum(dd) / k, the iteration's entry of `variance`; var < tol: converged, done */
__global__ void __launch_bounds__(64) k_bal_var(const double* __restrict__ dd, long long n, BalCtl* __restrict__ ctl, double tol, int max_iters,
                                                double* __restrict__ variance)
{
    const int done = ctl->done;
    __syncthreads();
    if (done) return;
    const double s = bal_vec_sum(dd, n, threadIdx.x);
    if (threadIdx.x != 0) return;
    const double var = s / ctl->k;
    const int it = ctl->n_iters;
    if (it < max_iters) variance[it] = var;
    ctl->n_iters = it + 1;
    if (var < tol) {
        ctl->converged = 1;
        ctl->done = 1;
    } else if (it + 1 >= max_iters)
        ctl->done = 1;
}
