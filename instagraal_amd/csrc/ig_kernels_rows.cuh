/* ig_kernels_rows.cuh -- the row builder: what the reports that sort contacts into rows share (the contacts in genome coordinates,
 * DESIGN.md 4.13; join support, 4.14; placement support, 4.16; the host side: ig_host_rows.inc).  A feature's own emit kernel runs
 * twice, a counting sort by row: it counts the entries per row, the 64-bit scan turns the counts into the rows' starts, it runs again
 * and every entry takes a slot of its row.  Then every row is sorted by column in one of three forms picked by the row's length
 * (k_lift_classify builds a work list per form):
 *   short  <= LIFT_SHORT_CAP entries: a wave per row, one entry per lane, a bitonic network of shuffles (k_lift_sort_wave)
 *   lds    <= LIFT_LDS_CAP entries:   a workgroup per row, a bitonic network in LDS (k_lift_sort_lds)
 *   long   anything else:             runs of the lds limit sorted by k_lift_sort_lds, then merged pairwise through a scratch
 *                                     buffer, every entry finding its place in the merged run by a binary search (k_lift_merge)
 * An entry is ONE 64-bit word, column << 32 | count, and the networks and merges order whole words: the order inside a row after
 * the scatter depends on how the atomics landed, the order after the sort does not (equal columns are ordered by their counts).
 * Where a feature asks for it the runs of equal columns are then summed (k_lift_row_bits, k_lift_head_totals, k_lift_reduce):
 * integer sums.  The kernels keep the names of the report they were written for.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define SCAN_THREADS 256
#define SCAN_ITEMS 8 /* words per thread of the scan */
#define SCAN_CHUNK (SCAN_THREADS * SCAN_ITEMS)

/* ---- the 64-bit inclusive prefix sums of arrays of 64-bit words (blockIdx.y: the array), in three steps: the totals of chunks of
 * SCAN_CHUNK words, an exclusive scan of the totals by one workgroup, every chunk scanned again from its total.  No workgroup waits
 * for another.  Besides the row builder the junction profile and the expected map run it (scan64_enqueue, ig_host_rows.inc). */

/* exclusive prefix of v over the workgroup's threads, and the total; wsum: SCAN_THREADS / 64 words of LDS */
__device__ __forceinline__ unsigned long long scan64_block(unsigned long long v, unsigned long long* wsum, unsigned long long* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads(); /* (whoever called before has read wsum) */
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < SCAN_THREADS / 64; k++) {
        const unsigned long long s = wsum[k];
        if (k < wave) before += s;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan64_totals(const unsigned long long* __restrict__ in, long long stride, int n,
                                                                unsigned long long* __restrict__ totals)
{
    __shared__ unsigned long long wsum[SCAN_THREADS / 64];
    const unsigned long long* a = in + (long long)blockIdx.y * stride;
    const int base = blockIdx.x * SCAN_CHUNK;
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const int idx = base + i * SCAN_THREADS + threadIdx.x;
        if (idx < n) v += a[idx];
    }
    unsigned long long total;
    scan64_block(v, wsum, &total);
    if (threadIdx.x == 0) totals[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan64_tops(unsigned long long* __restrict__ totals, int n_chunks)
{
    __shared__ unsigned long long wsum[SCAN_THREADS / 64];
    unsigned long long* t = totals + (size_t)blockIdx.x * n_chunks;
    unsigned long long carry = 0;
    for (int base = 0; base < n_chunks; base += SCAN_THREADS) {
        const int i = base + threadIdx.x;
        unsigned long long total;
        const unsigned long long ex = scan64_block(i < n_chunks ? t[i] : 0ull, wsum, &total);
        if (i < n_chunks) t[i] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan64_apply(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                               long long stride, int n, const unsigned long long* __restrict__ totals)
{
    __shared__ unsigned long long wsum[SCAN_THREADS / 64];
    const unsigned long long* a = in + (long long)blockIdx.y * stride;
    unsigned long long* o = out + (long long)blockIdx.y * stride;
    const int first = blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_ITEMS; /* SCAN_ITEMS words in a row per thread */
    unsigned long long w[SCAN_ITEMS], v = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        w[i] = first + i < n ? a[first + i] : 0ull;
        v += w[i];
    }
    unsigned long long total;
    unsigned long long run = totals[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + scan64_block(v, wsum, &total);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        run += w[i];
        if (first + i < n) o[first + i] = run;
    }
}

#define LIFT_THREADS 256
#define LIFT_SHORT_CAP 64  /* the wave form holds one entry per lane */
#define LIFT_LDS_CAP 1024  /* entries of the workgroup form: 8 KiB of LDS, so that LDS does not limit the eight workgroups (32 waves) of a CU;
                            * at cfg3 / cfg3_late no row of the fresh genome is longer than 841 */
/* RowBuf.sc's classify words, written by k_lift_classify: rows and entries per form, the runs of the long rows, their longest */
#define LIFT_C_SHORT_ROWS 0
#define LIFT_C_SHORT_ENT 1
#define LIFT_C_LDS_ROWS 2
#define LIFT_C_LDS_ENT 3
#define LIFT_C_LONG_ROWS 4
#define LIFT_C_LONG_ENT 5
#define LIFT_C_RUNS 6
#define LIFT_C_MAX_LONG 7
#define LIFT_C_WORDS 8
#define LIFT_PAD (~0ull) /* behind every real entry: a column is below 2^31 */

struct LiftItem { /* a stretch of the entries one workgroup sorts: a row of the lds form, or a run of a long row */
    long long off;
    int len, pad;
};
struct LiftLong { /* a long row: where it lies in the entries, in the scratch buffer, its length */
    long long off, scratch;
    long long len;
};

__device__ __forceinline__ unsigned long long lift_pack(int col, int cnt) { return ((unsigned long long)(unsigned)col << 32) | (unsigned long long)(unsigned)cnt; }

/* ---- the slot idiom of an emit kernel (k_lift_pass, k_join_emit; the scalars' head and tail are class_zero and class_flush) */

/* The combined form of taking a slot in row lo (lo < 0: the lane has no entry; whole waves call together): a run of a wave's lanes
 * with an equal lo (wave_runs, ig_kernels_wave.cuh) issues ONE atomic, by its head and for the run's length, and its lanes
 * take consecutive slots from what the head drew -- neighbouring words, written together.  counter: the rows' counts (SCATTER =
 * false: the returned slot means nothing) or their cursors (SCATTER = true).  The yardstick, one atomic per entry, is one line and
 * stays in the kernels, where the compiler nests the scatter's store under the atomic's own test. */
template <bool SCATTER>
__device__ __forceinline__ unsigned long long rows_slot(unsigned long long* counter, int lo, int lane)
{
    const WaveRuns r = wave_runs(lo, lane);
    unsigned long long base = 0;
    if (r.head && lo >= 0) base = atomicAdd(&counter[lo], (unsigned long long)(r.run_end - lane));
    if (!SCATTER) return 0ull;
    const unsigned long long upto = lane == 63 ? r.heads : r.heads & ((2ull << lane) - 1ull); /* (lane 0 is a head) */
    const int start = 63 - __clzll((long long)upto); /* the head of this lane's run */
    return __shfl(base, start, 64) + (unsigned long long)(lane - start);
}

/* The work lists of the three forms from the rows' lengths.  FILL = false: the sizes only (cls[]); FILL = true: the lists, each
 * row taking the next place of its list (cur[]: cursors; the order inside a list is free).  A long row is cut into runs of `run`
 * entries (run == 1: no run needs sorting).  short_max <= LIFT_SHORT_CAP, lds_max <= LIFT_LDS_CAP. */
template <bool FILL>
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_classify(const unsigned long long* __restrict__ rowstart, int U, int short_max, int lds_max,
                                                                unsigned long long* __restrict__ cls, unsigned long long* __restrict__ cur,
                                                                int* __restrict__ short_rows, LiftItem* __restrict__ lds_items,
                                                                LiftItem* __restrict__ run_items, LiftLong* __restrict__ long_rows)
{
    const int r = blockIdx.x * LIFT_THREADS + threadIdx.x;
    if (r >= U) return;
    const unsigned long long b = rowstart[r], len = rowstart[r + 1] - b;
    if (len < 2) return; /* sorted as it is */
    if (len <= (unsigned long long)short_max) {
        if (!FILL) {
            atomicAdd(&cls[LIFT_C_SHORT_ROWS], 1ull);
            atomicAdd(&cls[LIFT_C_SHORT_ENT], len);
        } else
            short_rows[atomicAdd(&cur[0], 1ull)] = r;
    } else if (len <= (unsigned long long)lds_max) {
        if (!FILL) {
            atomicAdd(&cls[LIFT_C_LDS_ROWS], 1ull);
            atomicAdd(&cls[LIFT_C_LDS_ENT], len);
        } else
            lds_items[atomicAdd(&cur[1], 1ull)] = LiftItem{(long long)b, (int)len, 0};
    } else {
        const unsigned long long run = (unsigned long long)lds_max;
        const unsigned long long n_runs = run > 1 ? (len + run - 1) / run : 0ull;
        if (!FILL) {
            atomicAdd(&cls[LIFT_C_LONG_ROWS], 1ull);
            atomicAdd(&cls[LIFT_C_LONG_ENT], len);
            if (n_runs) atomicAdd(&cls[LIFT_C_RUNS], n_runs);
            atomicMax(&cls[LIFT_C_MAX_LONG], len);
        } else {
            const unsigned long long at = atomicAdd(&cur[2], 1ull), scratch = atomicAdd(&cur[3], len);
            long_rows[at] = LiftLong{(long long)b, (long long)scratch, (long long)len};
            if (n_runs) {
                const unsigned long long first = atomicAdd(&cur[4], n_runs);
                for (unsigned long long q = 0; q < n_runs; q++) {
                    const unsigned long long o = q * run;
                    run_items[first + q] = LiftItem{(long long)(b + o), (int)(len - o < run ? len - o : run), 0};
                }
            }
        }
    }
}

/* the short form: a wave per listed row, an entry per lane (the others hold LIFT_PAD), a bitonic network over the wave */
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_sort_wave(const int* __restrict__ rows, int n_rows, const unsigned long long* __restrict__ rowstart,
                                                                 unsigned long long* __restrict__ ent)
{
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * (LIFT_THREADS / 64) + (threadIdx.x >> 6);
    if (item >= n_rows) return; /* (whole waves leave together) */
    const int r = rows[item];
    const unsigned long long b = rowstart[r];
    const int len = (int)min(rowstart[r + 1] - b, (unsigned long long)LIFT_SHORT_CAP);
    unsigned long long v = lane < len ? ent[b + lane] : LIFT_PAD;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(v, j, 64);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_min ? (o < v ? o : v) : (o > v ? o : v);
        }
    }
    if (lane < len) ent[b + lane] = v;
}

/* the lds form: a workgroup per listed stretch of at most LIFT_LDS_CAP entries, padded to a power of two, a bitonic network in LDS */
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_sort_lds(const LiftItem* __restrict__ items, unsigned long long* __restrict__ ent)
{
    __shared__ unsigned long long buf[LIFT_LDS_CAP];
    const LiftItem it = items[blockIdx.x];
    const int len = min(it.len, LIFT_LDS_CAP);
    int n2 = 2;
    while (n2 < len) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += LIFT_THREADS) buf[i] = i < len ? ent[it.off + i] : LIFT_PAD;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n2; t += LIFT_THREADS) {
                const int x = t ^ j;
                if (x > t) {
                    const unsigned long long a = buf[t], b = buf[x];
                    if ((a > b) == ((t & k) == 0)) {
                        buf[t] = b;
                        buf[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < len; i += LIFT_THREADS) ent[it.off + i] = buf[i];
}

/* One merge step of the long form (blockIdx.x: the long row; the workgroups of blockIdx.y share its entries): the sorted runs of
 * `width` entries are merged in pairs.  An entry of the left run goes to its index there plus the entries of the right run below
 * it, an entry of the right run to its index plus the entries of the left run not above it: every place is taken once, whatever
 * the words.  A run without a partner is copied.  to_scratch: from the entries to the scratch buffer, else back. */
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_merge(const LiftLong* __restrict__ rows, unsigned long long* __restrict__ ent,
                                                             unsigned long long* __restrict__ scratch, long long width, int to_scratch)
{
    const LiftLong row = rows[blockIdx.x];
    const unsigned long long* src = to_scratch ? ent + row.off : scratch + row.scratch;
    unsigned long long* dst = to_scratch ? scratch + row.scratch : ent + row.off;
    const long long stride = (long long)gridDim.y * LIFT_THREADS;
    for (long long e = (long long)blockIdx.y * LIFT_THREADS + threadIdx.x; e < row.len; e += stride) {
        const long long a0 = e / (2 * width) * (2 * width);
        const long long a1 = min(a0 + width, row.len), b1 = min(a0 + 2 * width, row.len);
        const unsigned long long v = src[e];
        long long lo, hi, at;
        if (e < a1) { /* left run: the entries of [a1, b1) below v */
            lo = a1, hi = b1;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (src[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            at = e + (lo - a1);
        } else { /* right run: the entries of [a0, a1) not above v */
            lo = a0, hi = a1;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (src[mid] <= v) lo = mid + 1;
                else hi = mid;
            }
            at = a0 + (e - a1) + (lo - a0);
        }
        dst[at] = v;
    }
}

/* ---- the reduction: the runs of equal columns inside a row become one entry each.  An entry is a HEAD if it is the first of its row
 * (a bit per entry, set from the rows' starts) or its column differs from the entry in front.  In chunks of SCAN_CHUNK entries:
 * the heads per chunk, their exclusive scan (k_scan64_tops), then every entry adds its count to the output entry of its run. */

__global__ void __launch_bounds__(LIFT_THREADS) k_lift_row_bits(const unsigned long long* __restrict__ rowstart, int U, unsigned* __restrict__ bits)
{
    const int r = blockIdx.x * LIFT_THREADS + threadIdx.x;
    if (r >= U) return;
    const unsigned long long b = rowstart[r];
    if (rowstart[r + 1] > b) atomicOr(&bits[b >> 5], 1u << (b & 31));
}

__device__ __forceinline__ bool lift_is_head(const unsigned long long* __restrict__ ent, const unsigned* __restrict__ bits, long long e)
{
    return ((bits[e >> 5] >> (e & 31)) & 1u) || (ent[e] >> 32) != (ent[e - 1] >> 32); /* (the first entry of all has its bit) */
}

__global__ void __launch_bounds__(SCAN_THREADS) k_lift_head_totals(const unsigned long long* __restrict__ ent, const unsigned* __restrict__ bits,
                                                                   long long n, unsigned long long* __restrict__ totals,
                                                                   unsigned long long* __restrict__ n_heads)
{
    __shared__ unsigned long long wsum[SCAN_THREADS / 64];
    const long long first = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_ITEMS;
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++)
        if (first + i < n && lift_is_head(ent, bits, first + i)) v++;
    unsigned long long total;
    scan64_block(v, wsum, &total);
    if (threadIdx.x == 0) {
        totals[blockIdx.x] = total;
        if (total) atomicAdd(n_heads, total);
    }
}

/* totals: scanned.  The head of run g writes its column, every entry of the run adds its count to out_cnt[g] (zeroed before), and
 * a head counts for its row (row_heads, zeroed before; the row of an entry by a binary search over the rows' starts): the scan of
 * row_heads gives the rows of the result. */
__global__ void __launch_bounds__(SCAN_THREADS) k_lift_reduce(const unsigned long long* __restrict__ ent, const unsigned* __restrict__ bits, long long n,
                                                              const unsigned long long* __restrict__ totals, const unsigned long long* __restrict__ rowstart,
                                                              int U, unsigned long long n_out, int* __restrict__ out_col,
                                                              unsigned long long* __restrict__ out_cnt, unsigned long long* __restrict__ row_heads)
{
    __shared__ unsigned long long wsum[SCAN_THREADS / 64];
    const long long first = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_ITEMS;
    bool head[SCAN_ITEMS];
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        head[i] = first + i < n && lift_is_head(ent, bits, first + i);
        v += head[i] ? 1ull : 0ull;
    }
    unsigned long long total;
    unsigned long long run = totals[blockIdx.x] + scan64_block(v, wsum, &total); /* heads in front of this thread's entries */
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const long long e = first + i;
        if (e >= n) break;
        if (head[i]) run++;
        const unsigned long long g = run - 1ull; /* (the first entry of all is a head: run >= 1) */
        if (run == 0ull || g >= n_out) continue;
        const unsigned long long w = ent[e];
        atomicAdd(&out_cnt[g], (unsigned long long)(long long)(int)(unsigned)(w & 0xffffffffull));
        if (head[i]) {
            out_col[g] = (int)(w >> 32);
            int lo = 0, hi = U; /* the last row that starts at or in front of e */
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (rowstart[mid] <= (unsigned long long)e) lo = mid;
                else hi = mid;
            }
            atomicAdd(&row_heads[lo], 1ull);
        }
    }
}

/* ---- the tests' own emit kernel (ig_debug_rows_build): the row builder over caller data, shaped like k_lift_pass.  Entry k goes to
 * row lo[k] (negative: no entry) as the word word[k]; the one scalar is the number of entries.  COMBINE = true: whole waves stay in
 * the loop and take their slots through rows_slot; false: one atomic per entry. */
template <bool SCATTER, bool COMBINE>
__global__ void __launch_bounds__(LIFT_THREADS) k_debug_rows_emit(const int* __restrict__ row, const unsigned long long* __restrict__ word, long long n,
                                                                  unsigned long long* __restrict__ counter, unsigned long long* __restrict__ ent,
                                                                  unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[1];
    if (!SCATTER) class_zero<1>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_ent = 0;
    const long long stride = (long long)gridDim.x * LIFT_THREADS;
    const long long nr = COMBINE ? (n + 63) & ~63LL : n; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x; k < nr; k += stride) {
        int lo = -1;
        if (k < n && row[k] >= 0) {
            lo = row[k];
            r_ent++;
        }
        unsigned long long slot = 0;
        if (!COMBINE) {
            if (lo >= 0) slot = atomicAdd(&counter[lo], 1ull);
        } else
            slot = rows_slot<SCATTER>(counter, lo, lane);
        if (SCATTER && lo >= 0 && slot < n_ent) ent[slot] = word[k];
    }
    if (SCATTER) return;
    if (r_ent) atomicAdd(&sc[0], r_ent);
    class_flush<1>(sc, out_sc);
}

/* ---- the tests' kernel over wave_runs / wave_run_sum (ig_debug_wave_runs), shaped like the combined loop of k_junc_observed: entry
 * k adds val[k] to out[key[k]] (a negative key: no entry), a run of a wave's lanes with an equal key through ONE atomic, by its
 * head, none where the run's values sum to 0.  *n_atomics: the atomics issued.  V: the type the sums are made in. */
template <typename V>
__global__ void __launch_bounds__(LIFT_THREADS) k_debug_wave_runs(const int* __restrict__ key, const long long* __restrict__ val, long long n,
                                                                  unsigned long long* __restrict__ out, unsigned long long* __restrict__ n_atomics)
{
    const int lane = threadIdx.x & 63;
    unsigned long long issued = 0;
    const long long stride = (long long)gridDim.x * LIFT_THREADS;
    const long long nr = (n + 63) & ~63LL; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x; k < nr; k += stride) {
        const int dest = k < n ? key[k] : -1;
        V v = dest >= 0 ? (V)val[k] : (V)0;
        const WaveRuns runs = wave_runs(dest, lane);
        v = wave_run_sum<V>(runs, v, lane);
        if (runs.head && dest >= 0 && v != 0) {
            atomicAdd(&out[dest], (unsigned long long)(long long)v);
            issued++;
        }
    }
    issued = wave_sum_u64(issued);
    if (lane == 0 && issued) atomicAdd(n_atomics, issued);
}
