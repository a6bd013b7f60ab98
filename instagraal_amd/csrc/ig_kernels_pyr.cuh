/* ig_kernels_pyr.cuh -- the contact levels of the pyramid: a level is the upper-triangular sum of a contact list,
 * rows ascending, columns ascending, 64-bit sums; the next level is the current one re-indexed through a table (lut[old] = new, or -1
 * for a fragment the filter destroyed) and summed again.  The rule is stated once, in instagraal_amd/pyramid_levels.py; the passes
 * here reproduce its arrays word for word.
 *
 * Here: k_pyr_canon (is the uploaded list its own level?), k_pyr_emit (the emit kernel of the row builder: over the uploaded list or
 * over the rows of the current level), k_pyr_largest (the largest sum of a level and the first pixel at or beyond 2^31),
 * k_pyr_degrees (the partners of every fragment) and k_pyr_expand (a stretch of a level as three int32 rows).
 *
 * Nothing here reads or writes anything a move reads or writes. */
#pragma once

#define PYR_THREADS 256
#define PYR_NS 4 /* the scalars k_pyr_emit sums */
#define PYR_IN 0
#define PYR_SKIPPED 1
#define PYR_DROPPED 2
#define PYR_KEPT 3
#define PYR_LIMIT 0x80000000ull /* pyramid_levels.LIMIT: a sum at or beyond it is refused */

/* the row of entry e of a level: the last row that starts at or in front of e (an empty row starts where the next one does) */
__device__ __forceinline__ int pyr_row_of(const unsigned long long* __restrict__ rowptr, int U, long long e)
{
    int lo = 0, hi = U;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rowptr[mid] <= (unsigned long long)e) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* out_sc[0]: the entries that break the canonical order: a > b, or (a, b) not behind the pair in front of it */
__global__ void __launch_bounds__(PYR_THREADS) k_pyr_canon(const int* __restrict__ a, const int* __restrict__ b, long long n, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[1];
    class_zero<1>(sc);
    unsigned long long r_bad = 0;
    const long long stride = (long long)gridDim.x * PYR_THREADS;
    for (long long k = (long long)blockIdx.x * PYR_THREADS + threadIdx.x; k < n; k += stride) {
        const int x = a[k], y = b[k];
        bool bad = x > y;
        if (k > 0) {
            const int px = a[k - 1], py = b[k - 1];
            bad = bad || px > x || (px == x && py >= y);
        }
        if (bad) r_bad++;
    }
    if (r_bad) atomicAdd(&sc[0], r_bad);
    class_flush<1>(sc, out_sc);
}

/* The emit kernel of a level: one pass over the n entries of its source, twice (the counting sort of the row builder).  RAW: the
 * source is the uploaded list (a, b, cnt) in file order; else the rows of the current level (rowptr[U_old + 1], col, sum: the row of
 * an entry from rowptr).  The first `skip` entries of the source are passed over (Q-P1); both ends go through lut (null: as they are)
 * and an entry with an end at -1 is dropped; what is left is an entry (row min, word max << 32 | count).  out_sc: PYR_NS scalars. */
template <bool SCATTER, bool RAW>
__global__ void __launch_bounds__(PYR_THREADS) k_pyr_emit(const int* __restrict__ a, const int* __restrict__ b, const int* __restrict__ cnt,
                                                          const unsigned long long* __restrict__ rowptr, const int* __restrict__ col,
                                                          const unsigned long long* __restrict__ sum, long long n, int U_old, const int* __restrict__ lut, int U_new,
                                                          long long skip, unsigned long long* __restrict__ counter, unsigned long long* __restrict__ ent,
                                                          unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[PYR_NS];
    if (!SCATTER) class_zero<PYR_NS>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_in = 0, r_skip = 0, r_drop = 0, r_kept = 0;
    const long long stride = (long long)gridDim.x * PYR_THREADS;
    const long long nr = (n + 63) & ~63LL;
    for (long long k = (long long)blockIdx.x * PYR_THREADS + threadIdx.x; k < nr; k += stride) {
        int lo = -1, hi = 0, w = 0;
        if (k < n) {
            r_in++;
            if (k < skip) r_skip++;
            else {
                int x, y, v;
                if (RAW) x = a[k], y = b[k], v = cnt[k];
                else x = pyr_row_of(rowptr, U_old, k), y = col[k], v = (int)sum[k];
                const bool inside = x >= 0 && y >= 0 && x < U_old && y < U_old;
                if (inside && lut) x = lut[x], y = lut[y];
                if (!inside || x < 0 || y < 0 || x >= U_new || y >= U_new) r_drop++;
                else {
                    lo = x < y ? x : y;
                    hi = x < y ? y : x;
                    w = v;
                    r_kept++;
                }
            }
        }
        const unsigned long long slot = rows_slot<SCATTER>(counter, lo, lane);
        if (SCATTER && lo >= 0 && slot < n_ent) ent[slot] = lift_pack(hi, w);
    }
    if (SCATTER) return;
    if (r_in) atomicAdd(&sc[PYR_IN], r_in);
    if (r_skip) atomicAdd(&sc[PYR_SKIPPED], r_skip);
    if (r_drop) atomicAdd(&sc[PYR_DROPPED], r_drop);
    if (r_kept) atomicAdd(&sc[PYR_KEPT], r_kept);
    class_flush<PYR_NS>(sc, out_sc);
}

/* largest: the largest sum of the level (a word that only grows); first_bad: the first pixel whose sum is 2^31 or more (the word
 * starts at ~0).  Whole waves. */
__global__ void __launch_bounds__(PYR_THREADS) k_pyr_largest(const unsigned long long* __restrict__ sum, long long n, unsigned long long* __restrict__ largest,
                                                             unsigned long long* __restrict__ first_bad)
{
    const int lane = threadIdx.x & 63;
    unsigned long long mx = 0;
    const long long stride = (long long)gridDim.x * PYR_THREADS;
    for (long long k = (long long)blockIdx.x * PYR_THREADS + threadIdx.x; k < n; k += stride) {
        const unsigned long long v = sum[k];
        mx = v > mx ? v : mx;
        if (v >= PYR_LIMIT) atomicMin(first_bad, (unsigned long long)k);
    }
    mx = wave_max_u64(mx);
    if (lane == 0 && mx) raise_max(largest, mx);
}

/* deg[i] (zeroed before): the j with (M + M^T)[i, j] != 0.  A run of a wave's lanes in one row adds its non-zero entries to the
 * row's degree with one atomic; every off-diagonal non-zero entry adds one to its column's.  Whole waves. */
__global__ void __launch_bounds__(PYR_THREADS) k_pyr_degrees(const unsigned long long* __restrict__ rowptr, int U, const int* __restrict__ col,
                                                             const unsigned long long* __restrict__ sum, long long n, unsigned* __restrict__ deg)
{
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * PYR_THREADS;
    const long long nr = (n + 63) & ~63LL;
    for (long long k = (long long)blockIdx.x * PYR_THREADS + threadIdx.x; k < nr; k += stride) {
        int row = -1, c = -1, nz = 0;
        if (k < n) {
            row = pyr_row_of(rowptr, U, k);
            c = col[k];
            nz = sum[k] != 0ull ? 1 : 0;
        }
        const WaveRuns r = wave_runs(row, lane);
        const int s = wave_run_sum(r, nz, lane);
        if (r.head && row >= 0 && s) atomicAdd(&deg[row], (unsigned)s);
        if (nz && c != row && c >= 0 && c < U) atomicAdd(&deg[c], 1u);
    }
}

/* the entries first .. first + n - 1 of a level as data3's three rows: the row ids are expanded here */
__global__ void __launch_bounds__(PYR_THREADS) k_pyr_expand(const unsigned long long* __restrict__ rowptr, int U, const int* __restrict__ col,
                                                            const unsigned long long* __restrict__ sum, long long first, long long n, int* __restrict__ out_row,
                                                            int* __restrict__ out_col, int* __restrict__ out_cnt)
{
    const long long stride = (long long)gridDim.x * PYR_THREADS;
    for (long long k = (long long)blockIdx.x * PYR_THREADS + threadIdx.x; k < n; k += stride) {
        const long long e = first + k;
        out_row[k] = pyr_row_of(rowptr, U, e);
        out_col[k] = col[e];
        out_cnt[k] = (int)sum[e];
    }
}
