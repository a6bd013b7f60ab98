/* ig_kernels_pairs.cuh -- read pairs lifted onto the current genome: every Hi-C read pair, aligned to the input
 * contigs, re-expressed in the coordinates of the scaffolds as they stand; the kept pairs stay on the device (the STORE), and from
 * them come the pixels at any unit and the distance histogram per strand combination.  The rule is stated once, in
 * instagraal_amd/pairs_lift.py; the passes here reproduce its arrays byte for byte.
 *
 * Here: k_pairs_lift (one pair per thread, two binary searches, the wave-aggregated append), k_pairs_emit (the feature's emit kernel
 * for the row builder: count, then scatter; ig_kernels_rows.cuh does the rest) and k_pairs_law (an LDS histogram per workgroup).
 *
 * Nothing here reads or writes anything a move reads or writes. */
#pragma once

#define PAIRS_THREADS 256
#define PAIRS_NS 5           /* the scalars k_pairs_lift sums: the order of ig_pairs_lift's scalars[0..4] (pairs_lift.SCALARS) */
#define PAIRS_IN 0
#define PAIRS_KEPT 1
#define PAIRS_MISS1 2
#define PAIRS_MISS2 3
#define PAIRS_UNPLACED 4
#define PAIRS_MAX_EDGES 512
#define PAIRS_KIND_SUB 0     /* pairs_lift.UNIT_KINDS */
#define PAIRS_KIND_BIN 1
#define PAIRS_KIND_BINSIZE 2
#define PAIRS_KIND_SCAFFOLD 3
/* a stored pair's flag byte */
#define PAIRS_F_REV1 1       /* end 1 lies on a reversed interval */
#define PAIRS_F_REV2 2
#define PAIRS_F_MINUS1 4     /* end 1 was read on '-' */
#define PAIRS_F_MINUS2 8

/* one interval of the source table, gathered once per end; its start is the word the search found */
struct PairsIv {
    int src_end;   /* exclusive */
    int new_start; /* inside its scaffold */
    int scaf_rev;  /* scaffold << 1 | reversed; negative: the sub-fragment is not placed */
    int position;  /* of the sub-fragment in the genome order, -1 */
};

/* what the caller may ask back per pair, in input order (every pointer may be null together: out.status == nullptr) */
struct PairsOut {
    int *scaffold1, *pos1, *unit1, *scaffold2, *pos2, *unit2;
    unsigned char *rev1, *rev2, *status;
};

/* the store: the kept pairs, in no particular order */
struct PairsStore {
    int4* ends;          /* (scaffold 1, 0-based position 1, scaffold 2, 0-based position 2) */
    int2* unit;          /* the positions of the two intervals in the genome order */
    unsigned char* flag; /* PAIRS_F_* */
};

struct PairsEnd {
    bool hit;
    int scaffold, new0, unit, rev;
};

/* One end: contig c, 1-based position p.  start[rowptr[c] .. rowptr[c + 1]) are the starts of contig c's intervals, ascending. */
__device__ __forceinline__ PairsEnd pairs_lift_end(int c, int p, const int* __restrict__ rowptr, int n_contigs, const int* __restrict__ start,
                                                   const PairsIv* __restrict__ iv)
{
    PairsEnd e = {false, -1, 0, -1, 0};
    if (c < 0 || c >= n_contigs || p < 1) return e;
    const int pos0 = p - 1;
    int lo = rowptr[c], hi = rowptr[c + 1]; /* the first interval whose start is beyond pos0 lies in [lo, hi] */
    const int first = lo;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (start[mid] <= pos0) lo = mid + 1;
        else hi = mid;
    }
    const int i = lo - 1;
    if (i < first) return e;
    const PairsIv v = iv[i];
    if (pos0 >= v.src_end) return e;
    e.hit = true;
    if (v.scaf_rev < 0) return e;
    const int s = start[i], off = pos0 - s;
    e.rev = v.scaf_rev & 1;
    e.scaffold = v.scaf_rev >> 1;
    e.new0 = v.new_start + (e.rev ? v.src_end - s - 1 - off : off);
    e.unit = v.position;
    return e;
}

/* One pair per thread.  The per-pair outputs go to the caller's arrays in input order; a kept pair is appended to the store behind
 * *cursor: the kept lanes of a wave are counted by a ballot, one lane draws their places with one atomic and every kept lane takes
 * the place of its rank among them (the order inside the store is free: everything built from it is a sum).  cap: the store's
 * capacity -- nothing is written beyond it.  The five scalars: a ballot each, one atomic per wave and non-zero count. */
__global__ void __launch_bounds__(PAIRS_THREADS) k_pairs_lift(const int* __restrict__ c1, const int* __restrict__ p1, const int* __restrict__ c2,
                                                              const int* __restrict__ p2, const unsigned char* __restrict__ strands, long long n,
                                                              const int* __restrict__ rowptr, int n_contigs, const int* __restrict__ start,
                                                              const PairsIv* __restrict__ iv, PairsOut out, PairsStore store,
                                                              unsigned long long* __restrict__ cursor, unsigned long long cap,
                                                              unsigned long long* __restrict__ out_sc)
{
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * PAIRS_THREADS;
    const long long nr = (n + 63) & ~63LL; /* whole waves stay in the loop together (the ballots need every lane) */
    unsigned long long w_in = 0, w_kept = 0, w_m1 = 0, w_m2 = 0, w_un = 0; /* per wave, the same in every lane */
    for (long long k = (long long)blockIdx.x * PAIRS_THREADS + threadIdx.x; k < nr; k += stride) {
        const bool live = k < n;
        int status = -1;
        PairsEnd a = {false, -1, 0, -1, 0}, b = a;
        if (live) {
            a = pairs_lift_end(c1[k], p1[k], rowptr, n_contigs, start, iv);
            b = pairs_lift_end(c2[k], p2[k], rowptr, n_contigs, start, iv);
            status = !a.hit ? 1 : !b.hit ? 2 : (a.scaffold < 0 || b.scaffold < 0) ? 3 : 0;
            if (out.status) {
                out.scaffold1[k] = a.scaffold, out.pos1[k] = a.scaffold < 0 ? 0 : a.new0 + 1, out.unit1[k] = a.unit, out.rev1[k] = (unsigned char)a.rev;
                out.scaffold2[k] = b.scaffold, out.pos2[k] = b.scaffold < 0 ? 0 : b.new0 + 1, out.unit2[k] = b.unit, out.rev2[k] = (unsigned char)b.rev;
                out.status[k] = (unsigned char)status;
            }
        }
        const unsigned long long kept = __ballot(status == 0);
        w_in += (unsigned long long)__popcll(__ballot(live));
        w_kept += (unsigned long long)__popcll(kept);
        w_m1 += (unsigned long long)__popcll(__ballot(status == 1));
        w_m2 += (unsigned long long)__popcll(__ballot(status == 2));
        w_un += (unsigned long long)__popcll(__ballot(status == 3));
        if (kept) { /* (the same in every lane) */
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(kept));
            base = __shfl(base, 0, 64);
            if (status == 0) {
                const unsigned long long slot = base + (unsigned long long)__popcll(kept & ((1ull << lane) - 1ull));
                if (slot < cap) {
                    const int sb = strands ? strands[k] : 0;
                    store.ends[slot] = make_int4(a.scaffold, a.new0, b.scaffold, b.new0);
                    store.unit[slot] = make_int2(a.unit, b.unit);
                    store.flag[slot] = (unsigned char)((a.rev ? PAIRS_F_REV1 : 0) | (b.rev ? PAIRS_F_REV2 : 0) | ((sb & 1) ? PAIRS_F_MINUS1 : 0) | ((sb & 2) ? PAIRS_F_MINUS2 : 0));
                }
            }
        }
    }
    if (lane == 0) {
        if (w_in) atomicAdd(&out_sc[PAIRS_IN], w_in);
        if (w_kept) atomicAdd(&out_sc[PAIRS_KEPT], w_kept);
        if (w_m1) atomicAdd(&out_sc[PAIRS_MISS1], w_m1);
        if (w_m2) atomicAdd(&out_sc[PAIRS_MISS2], w_m2);
        if (w_un) atomicAdd(&out_sc[PAIRS_UNPLACED], w_un);
    }
}

/* the unit of one end.  tab: "bin", the unit of every position; a bin size, the first unit of every scaffold */
__device__ __forceinline__ int pairs_unit(int kind, unsigned binsize, const int* __restrict__ tab, int scaffold, int new0, int position)
{
    if (kind == PAIRS_KIND_SUB) return position;
    if (kind == PAIRS_KIND_BIN) return tab[position];
    if (kind == PAIRS_KIND_SCAFFOLD) return scaffold;
    return tab[scaffold] + (int)((unsigned)new0 / binsize);
}

/* The emit kernel of the pixels: one pass over the store, twice (the counting sort of the row builder, as k_lift_pass).  A stored pair
 * is an entry (row lo = min unit, word hi << 32 | 1); out_sc[0]: the entries, out_sc[1]: pairs with a unit outside 0 .. U - 1 (none,
 * unless the tables are inconsistent: the host refuses the build then). */
template <bool SCATTER>
__global__ void __launch_bounds__(PAIRS_THREADS) k_pairs_emit(PairsStore store, long long n, int kind, unsigned binsize, const int* __restrict__ tab, int U,
                                                              unsigned long long* __restrict__ counter, unsigned long long* __restrict__ ent,
                                                              unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[2];
    if (!SCATTER) class_zero<2>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_ent = 0, r_bad = 0;
    const long long stride = (long long)gridDim.x * PAIRS_THREADS;
    const long long nr = (n + 63) & ~63LL;
    for (long long k = (long long)blockIdx.x * PAIRS_THREADS + threadIdx.x; k < nr; k += stride) {
        int lo = -1, hi = 0;
        if (k < n) {
            const int4 e = store.ends[k];
            int2 u = make_int2(0, 0);
            if (kind == PAIRS_KIND_SUB || kind == PAIRS_KIND_BIN) u = store.unit[k];
            const int a = pairs_unit(kind, binsize, tab, e.x, e.y, u.x), b = pairs_unit(kind, binsize, tab, e.z, e.w, u.y);
            if (a < 0 || b < 0 || a >= U || b >= U) r_bad++;
            else {
                lo = min(a, b);
                hi = max(a, b);
                r_ent++;
            }
        }
        const unsigned long long slot = rows_slot<SCATTER>(counter, lo, lane);
        if (SCATTER && lo >= 0 && slot < n_ent) ent[slot] = lift_pack(hi, 1);
    }
    if (SCATTER) return;
    if (r_ent) atomicAdd(&sc[0], r_ent);
    if (r_bad) atomicAdd(&sc[1], r_bad);
    class_flush<2>(sc, out_sc);
}

/* The distance histogram of the stored pairs with both ends on one scaffold: idx = clip(searchsorted(edges, |pos2 - pos1|, "right")
 * - 1, 0, n_edges - 2), by strand combination ++ +- -+ -- (flip: an end on a reversed interval has its strand flipped).  The edges
 * and a [4][n_edges - 1] histogram of 32-bit counters live in LDS; a workgroup sees fewer than 2^31 pairs (the store holds no more),
 * so no counter overflows; the flush is one 64-bit atomic per non-zero counter. */
__global__ void __launch_bounds__(PAIRS_THREADS) k_pairs_law(PairsStore store, long long n, const long long* __restrict__ edges, int n_edges, int flip,
                                                             unsigned long long* __restrict__ counts)
{
    __shared__ long long s_edge[PAIRS_MAX_EDGES];
    __shared__ unsigned s_hist[4 * (PAIRS_MAX_EDGES - 1)];
    const int nb = n_edges - 1;
    for (int i = threadIdx.x; i < n_edges; i += PAIRS_THREADS) s_edge[i] = edges[i];
    for (int i = threadIdx.x; i < 4 * nb; i += PAIRS_THREADS) s_hist[i] = 0u;
    __syncthreads();
    const long long stride = (long long)gridDim.x * PAIRS_THREADS;
    for (long long k = (long long)blockIdx.x * PAIRS_THREADS + threadIdx.x; k < n; k += stride) {
        const int4 e = store.ends[k];
        if (e.x != e.z) continue;
        const int f = store.flag[k];
        int s1 = (f & PAIRS_F_MINUS1) ? 1 : 0, s2 = (f & PAIRS_F_MINUS2) ? 1 : 0;
        if (flip) s1 ^= (f & PAIRS_F_REV1) ? 1 : 0, s2 ^= (f & PAIRS_F_REV2) ? 1 : 0;
        const long long d = e.w >= e.y ? (long long)e.w - e.y : (long long)e.y - e.w;
        int lo = 0, hi = n_edges; /* the first edge beyond d lies in [lo, hi] */
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_edge[mid] <= d) lo = mid + 1;
            else hi = mid;
        }
        const int idx = min(max(lo - 1, 0), nb - 1);
        atomicAdd(&s_hist[(s1 * 2 + s2) * nb + idx], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * nb; i += PAIRS_THREADS) {
        const unsigned v = s_hist[i];
        if (v) atomicAdd(&counts[i], (unsigned long long)v);
    }
}
