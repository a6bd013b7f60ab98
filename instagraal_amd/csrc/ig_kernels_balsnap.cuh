/* ig_kernels_balsnap.cuh -- the balancing's rows from a BUILT map (the rule: entries_of_rows, instagraal_amd/balance.py;
 * the host side: ig_host_balsnap.inc).  Every map the library builds stays on the device as a sorted, summed, upper-triangular
 * snapshot (LiftBuf: rowptr, out_col, out_cnt); k_balsnap_emit turns its entries into the rows k_bal_marginals iterates over
 * without a pass over the contacts: one thread per snapshot entry (u, v, c), its row u by a search of rowptr (zoom_row_of), the
 * three tests of the rule, and for a kept entry the two emissions (row u, column v) and (row v, column u) through the row builder's
 * counting sort (ig_kernels_rows.cuh).
 * The word of an emission is column << 32 | INDEX OF THE SNAPSHOT ENTRY, not its count: the kept entries of a row have distinct
 * columns, so the sort needs no rule for ties and nothing is left to sum -- the build has no reduction -- and k_balsnap_gather
 * fetches the 64-bit count through the index once the rows are sorted.  A count never passes through the low half of a word.
 * The snapshot is read only.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define BALSNAP_NS 5 /* the scalars the count pass owns: the order of ig_balance_build_snapshot's scalars[0..4] */
#define BALSNAP_WITHIN_OBS 0
#define BALSNAP_BAND_OBS 1
#define BALSNAP_OTHER_OBS 2
#define BALSNAP_KEPT_OBS 3
#define BALSNAP_ENTRIES 4

/* One pass over the K entries of the snapshot (rowptr [U + 1], col and cnt [K]), twice, shaped like k_bal_emit.  mode 0: every entry
 * outside the band is kept; 1 (cis): those with group[u] == group[v]; 2 (trans): those with group[u] != group[v] (group [U]; not
 * read at mode 0).  An entry whose column is not inside u .. U - 1 is no entry of an upper-triangular map and is left out of
 * everything (the host tells by the sum of the scalars).
 * SCATTER = false: an entry is classified by the first test it meets (u == v, v - u < ignore_diags, outside the mode, kept); a kept
 * one counts for the rows of both units and adds its count to their totals (64-bit integer atomics: the host refuses a total of 2^53
 * or more, and a built map's counts -- sums of 32-bit counts over fewer than 2^31 entries -- cannot wrap 64 bits on the way there).
 * SCATTER = true: the counters have become cursors; each of the two emissions takes the next slot of its row.
 * The upper emission goes to row u, and the entries of a row lie side by side in the snapshot: a wave's lanes hold long runs of one
 * u, which take their slots -- and add to total[u] -- through ONE atomic per run (rows_slot, wave_run_sum).  The mirrored emission
 * goes to row v, ascending strictly along such a run: one atomic each.  Whole waves stay in the loop (the shuffles need every lane). */
template <bool SCATTER>
__global__ void __launch_bounds__(LIFT_THREADS) k_balsnap_emit(const unsigned long long* __restrict__ rowptr, const int* __restrict__ col,
                                                               const unsigned long long* __restrict__ cnt, int U, long long K, int ignore_diags, int mode,
                                                               const int* __restrict__ group, unsigned long long* __restrict__ counter,
                                                               unsigned long long* __restrict__ total, unsigned long long* __restrict__ ent,
                                                               unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[BALSNAP_NS];
    if (!SCATTER) class_zero<BALSNAP_NS>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_within = 0, r_band = 0, r_other = 0, r_kept = 0, r_ent = 0;
    const long long stride = (long long)gridDim.x * LIFT_THREADS;
    const long long nr = (K + 63) & ~63LL;
    for (long long e = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x; e < nr; e += stride) {
        int u = -1, v = -1; /* u stays -1 where the lane has no kept entry */
        unsigned long long cv = 0;
        if (e < K) {
            const int row = zoom_row_of(rowptr, U, e);
            v = col[e];
            if (v >= row && v < U) {
                if (!SCATTER) cv = cnt[e];
                bool keep = false;
                if (v == row) r_within += cv;
                else if (v - row < ignore_diags) r_band += cv;
                else if (mode != 0 && (group[row] == group[v]) != (mode == 1)) r_other += cv;
                else keep = true;
                if (keep) u = row;
            }
        }
        const unsigned long long su = rows_slot<SCATTER>(counter, u, lane);
        if (!SCATTER) {
            const WaveRuns runs = wave_runs(u, lane);
            const long long run_total = wave_run_sum<long long>(runs, u >= 0 ? (long long)cv : 0ll, lane);
            if (runs.head && u >= 0 && run_total != 0) atomicAdd(&total[u], (unsigned long long)run_total);
            if (u >= 0) {
                r_kept += cv;
                r_ent += 2ull;
                atomicAdd(&counter[v], 1ull);
                if (cv) atomicAdd(&total[v], cv);
            }
        } else if (u >= 0) {
            const unsigned long long sv = atomicAdd(&counter[v], 1ull);
            const unsigned long long idx = (unsigned long long)e & 0xffffffffull;
            if (su < n_ent) ent[su] = ((unsigned long long)(unsigned)v << 32) | idx;
            if (sv < n_ent) ent[sv] = ((unsigned long long)(unsigned)u << 32) | idx;
        }
    }
    if (SCATTER) return;
    if (r_within) atomicAdd(&sc[BALSNAP_WITHIN_OBS], r_within);
    if (r_band) atomicAdd(&sc[BALSNAP_BAND_OBS], r_band);
    if (r_other) atomicAdd(&sc[BALSNAP_OTHER_OBS], r_other);
    if (r_kept) atomicAdd(&sc[BALSNAP_KEPT_OBS], r_kept);
    if (r_ent) atomicAdd(&sc[BALSNAP_ENTRIES], r_ent);
    class_flush<BALSNAP_NS>(sc, out_sc);
}

/* the sorted words become the rows' entries: out_col[e] = word >> 32, out_cnt[e] = the 64-bit count of the snapshot entry the word
 * names (an index beyond the snapshot reads nothing: 0) */
__global__ void __launch_bounds__(LIFT_THREADS) k_balsnap_gather(const unsigned long long* __restrict__ ent, long long E,
                                                                 const unsigned long long* __restrict__ snap_cnt, long long K, int* __restrict__ out_col,
                                                                 unsigned long long* __restrict__ out_cnt)
{
    const long long stride = (long long)gridDim.x * LIFT_THREADS;
    for (long long e = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x; e < E; e += stride) {
        const unsigned long long w = ent[e];
        const long long src = (long long)(w & 0xffffffffull);
        out_col[e] = (int)(w >> 32);
        out_cnt[e] = src < K ? snap_cnt[src] : 0ull;
    }
}
