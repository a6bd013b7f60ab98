/* ig_kernels_zoom.cuh -- fixed-resolution maps of the current genome (the rule: instagraal_amd/zoom_levels.py; the
 * host side: ig_host_zoom.inc): the lift with a caller's unit per position (k_zoom_keys in front of k_lift_pass and the row builder,
 * ig_kernels_rows.cuh), and the COARSENING of a built, reduced level: entry (lo, hi, c) goes to (map[lo], map[hi]), equal keys are
 * summed.  The map is non-decreasing, so coarse row R is a contiguous range of fine rows and hence of fine entries -- a SEGMENT --
 * and no counting sort is needed: the segments' starts are gathered from the fine rows (k_zoom_rowstart), every entry becomes the
 * word mapped column << 32 | index inside its segment (k_zoom_words), the row builder's three forms sort the segments, and the
 * reduction adds the fine 64-bit count found THROUGH the index to the run of its mapped column (k_zoom_reduce).  A count never passes
 * through the low half of a word, so it may exceed 2^32; the words of a segment are distinct, so the sort needs no rule for ties.
 *
 * Nothing here writes anything a move reads. */
#pragma once

/* the unit of every sub-fragment from the caller's table by position, -1: not placed (k_lift_keys' shape with an int32 table) */
__global__ void __launch_bounds__(LIFT_THREADS) k_zoom_keys(const int* __restrict__ pix, int M, int T, const int* __restrict__ unit, int* __restrict__ key)
{
    const int s = blockIdx.x * LIFT_THREADS + threadIdx.x;
    if (s >= M) return;
    const int p = pix[s];
    key[s] = (p >= 0 && p < T) ? unit[p] : -1;
}

/* segstart[R], R = 0 .. C: the first fine entry of coarse row R = rowptr[first fine row u with map[u] >= R] (rowptr[U] where there
 * is none).  Thread u = 0 .. U writes the coarse rows in (map[u - 1], map[u]] (map[-1] = -1, map[U] = C): every R once, the coarse
 * rows no fine row maps to included.  map: non-decreasing, inside 0 .. C - 1 (checked on the host). */
__global__ void __launch_bounds__(LIFT_THREADS) k_zoom_rowstart(const unsigned long long* __restrict__ rowptr, const int* __restrict__ map, int U, int C,
                                                                unsigned long long* __restrict__ segstart)
{
    const long long u = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x;
    if (u > U) return;
    const int prev = u == 0 ? -1 : map[u - 1];
    const int cur = u == U ? C : min(map[u], C);
    const unsigned long long v = rowptr[u];
    for (int R = prev + 1; R <= cur; R++) segstart[R] = v;
}

/* the last of n_rows rows that starts at or in front of entry e (start[0] = 0 <= e; n_rows >= 1) */
__device__ __forceinline__ int zoom_row_of(const unsigned long long* __restrict__ start, int n_rows, long long e)
{
    int lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= (unsigned long long)e) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* word[e] = map[col[e]] << 32 | e - segstart[map[fine row of e]].  A thread takes SCAN_ITEMS entries in a row: one binary search
 * for the fine row of the first, then a walk.  The index fits 32 bits: checked on the host from the segments' starts. */
__global__ void __launch_bounds__(LIFT_THREADS) k_zoom_words(const unsigned long long* __restrict__ rowptr, const int* __restrict__ col,
                                                             const int* __restrict__ map, int U, long long K,
                                                             const unsigned long long* __restrict__ segstart, unsigned long long* __restrict__ word)
{
    const long long first = ((long long)blockIdx.x * LIFT_THREADS + threadIdx.x) * SCAN_ITEMS;
    if (first >= K) return;
    int u = zoom_row_of(rowptr, U, first);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const long long e = first + i;
        if (e >= K) break;
        while (u + 1 < U && rowptr[u + 1] <= (unsigned long long)e) u++;
        const int hi = min(max(col[e], 0), U - 1);
        word[e] = ((unsigned long long)(unsigned)map[hi] << 32) | ((unsigned long long)e - segstart[map[u]]);
    }
}

/* k_lift_reduce over the sorted words of the segments, the count gathered through the index: the head of run g writes its mapped
 * column, every entry of the run adds fine_cnt[segstart[R] + index] to out_cnt[g] (zeroed before), and a head counts for its coarse
 * row R (row_heads, zeroed before).  totals: the scanned heads per chunk (k_lift_head_totals, k_scan64_tops).  A thread finds the
 * segment of its first entry by a binary search and walks from there. */
__global__ void __launch_bounds__(SCAN_THREADS) k_zoom_reduce(const unsigned long long* __restrict__ word, const unsigned* __restrict__ bits, long long n,
                                                              const unsigned long long* __restrict__ totals, const unsigned long long* __restrict__ segstart,
                                                              int C, const unsigned long long* __restrict__ fine_cnt, unsigned long long n_out,
                                                              int* __restrict__ out_col, unsigned long long* __restrict__ out_cnt,
                                                              unsigned long long* __restrict__ row_heads)
{
    __shared__ unsigned long long wsum[SCAN_THREADS / 64];
    const long long first = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_ITEMS;
    bool head[SCAN_ITEMS];
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        head[i] = first + i < n && lift_is_head(word, bits, first + i);
        v += head[i] ? 1ull : 0ull;
    }
    unsigned long long total;
    unsigned long long run = totals[blockIdx.x] + scan64_block(v, wsum, &total); /* heads in front of this thread's entries */
    if (first >= n) return;
    int R = zoom_row_of(segstart, C, first);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const long long e = first + i;
        if (e >= n) break;
        while (R + 1 < C && segstart[R + 1] <= (unsigned long long)e) R++;
        if (head[i]) run++;
        const unsigned long long g = run - 1ull; /* (the first entry of all is a head: run >= 1) */
        if (run == 0ull || g >= n_out) continue;
        const unsigned long long w = word[e];
        const unsigned long long src = segstart[R] + (w & 0xffffffffull);
        if (src < (unsigned long long)n) atomicAdd(&out_cnt[g], fine_cnt[src]);
        if (head[i]) {
            out_col[g] = (int)(w >> 32);
            atomicAdd(&row_heads[R], 1ull);
        }
    }
}
