/* ig_kernels_lift.cuh -- the contacts in the coordinates of the current genome: every uploaded contact re-indexed from sub-fragment
 * ids to UNITS of the genome order (level 0: the positions of the contact map; level 1: the placed bins in genome order), as a CSR
 * matrix of the upper triangle sorted by (row, column).  The rule is stated once, in instagraal_amd/assembly_contacts.py; the
 * passes here reproduce its arrays byte for byte.
 *
 * Here: the units (k_lift_heads, k_lift_keys) and the feature's emit kernel (k_lift_pass: count, then scatter).  The counting sort
 * around it, the sort of every row by column and, at level 1, the sum of the runs of equal columns are the row builder's
 * (ig_kernels_rows.cuh, rows_build in ig_host_rows.inc).
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define LIFT_NS 5          /* the scalars the passes over the contacts own: the order of ig_assembly_contacts_build's scalars[0..4] */
#define LIFT_ENTRIES_IN 0
#define LIFT_ENTRIES_KEPT 1
#define LIFT_CONTACTS_KEPT 2
#define LIFT_ENTRIES_UNPLACED 3
#define LIFT_CONTACTS_UNPLACED 4

/* level 1: head[r] = 1 where the parent bin changes along the order (position 0 included): their running sum less one is the unit */
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_heads(const SubTab* __restrict__ sub, const int* __restrict__ order, int T,
                                                             unsigned long long* __restrict__ head)
{
    const int r = blockIdx.x * LIFT_THREADS + threadIdx.x;
    if (r >= T) return;
    head[r] = (r == 0 || sub[order[r]].parent != sub[order[r - 1]].parent) ? 1ull : 0ull;
}

/* the unit of every sub-fragment, -1: not placed.  incl (level 1 only): the running sum of the heads by position */
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_keys(const int* __restrict__ pix, int M, int T, const unsigned long long* __restrict__ incl,
                                                            int* __restrict__ key)
{
    const int s = blockIdx.x * LIFT_THREADS + threadIdx.x;
    if (s >= M) return;
    const int p = pix[s];
    int u = -1;
    if (p >= 0 && p < T) u = incl ? (int)(incl[p] - 1ull) : p;
    key[s] = u;
}

/* One pass over the contacts (row of contact k: crow[k]; column and count: cc[k]), twice.
 * SCATTER = false: a kept contact counts for its row lo = min(unit, unit); the five scalars are summed in registers and reach
 * memory once per workgroup (as k_law_observed<true>).
 * SCATTER = true: the counters have become cursors that start at the rows' first entries; the contact takes the next slot of its
 * row and writes (hi, count) there.  n_ent: the entries the first pass counted -- nothing is written beyond them.
 * COMBINE = false, the yardstick: one atomic per kept contact.  COMBINE = true: the lanes of a wave hold 64 consecutive contacts,
 * mostly of one row of the input and so, wherever that row's sub-fragment lies in front of its partners, of one row of the result:
 * a run of lanes with an equal lo issues ONE atomic, by its head and for the run's length (rows_slot, ig_kernels_rows.cuh), and its
 * lanes take consecutive slots from what the head drew -- neighbouring words, written together.  Which slot an entry gets
 * inside its row differs between the forms and from run to run; the sort behind it makes the result the same.
 * A sharded handle takes the rows i % world == rank. */
template <bool SCATTER, bool COMBINE>
__global__ void __launch_bounds__(LIFT_THREADS) k_lift_pass(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                            const int* __restrict__ key, int U, unsigned long long* __restrict__ counter,
                                                            unsigned long long* __restrict__ ent, unsigned long long n_ent,
                                                            unsigned long long* __restrict__ out_sc, int rank, int world)
{
    __shared__ unsigned long long sc[LIFT_NS];
    if (!SCATTER) class_zero<LIFT_NS>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_in = 0, r_kept = 0, r_ckept = 0, r_unpl = 0, r_cunpl = 0;
    const long long stride = (long long)gridDim.x * LIFT_THREADS;
    const long long Zr = COMBINE ? (Z + 63) & ~63LL : Z; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x; k < Zr; k += stride) {
        int lo = -1, hi = 0, cnt = 0; /* lo = -1: nothing to place */
        if (k < Z) {
            const int i = crow[k];
            if (contact_is_mine(i, rank, world)) {
                const int2 e = cc[k];
                const int a = key[i], b = key[e.x];
                const unsigned long long cv = (unsigned long long)(long long)e.y;
                r_in++;
                if (a < 0 || b < 0 || a >= U || b >= U) {
                    r_unpl++;
                    r_cunpl += cv;
                } else {
                    r_kept++;
                    r_ckept += cv;
                    lo = min(a, b);
                    hi = max(a, b);
                    cnt = e.y;
                }
            }
        }
        unsigned long long slot = 0;
        if (!COMBINE) {
            if (lo >= 0) slot = atomicAdd(&counter[lo], 1ull);
        } else
            slot = rows_slot<SCATTER>(counter, lo, lane);
        if (SCATTER && lo >= 0 && slot < n_ent) ent[slot] = lift_pack(hi, cnt);
    }
    if (SCATTER) return;
    if (r_in) atomicAdd(&sc[LIFT_ENTRIES_IN], r_in);
    if (r_kept) atomicAdd(&sc[LIFT_ENTRIES_KEPT], r_kept);
    if (r_ckept) atomicAdd(&sc[LIFT_CONTACTS_KEPT], r_ckept);
    if (r_unpl) atomicAdd(&sc[LIFT_ENTRIES_UNPLACED], r_unpl);
    if (r_cunpl) atomicAdd(&sc[LIFT_CONTACTS_UNPLACED], r_cunpl);
    class_flush<LIFT_NS>(sc, out_sc);
}

