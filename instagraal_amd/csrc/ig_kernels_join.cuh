/* ig_kernels_join.cuh -- join support: the junction profile for junctions that do not exist yet.  For every pair of ENDS of the placed
 * contigs that are not rings (end e = 2 k + side of run k of the genome order; side 0: the head) the contacts that would span the
 * join inside a window of w positions, the sub-fragment pairs that could, and what the model in use would expect of them if the
 * two ends were adjacent.  The rule is stated once, in instagraal_amd/join_support.py; the passes here reproduce its arrays byte
 * for byte.
 *
 * The ends: k_join_heads flags the first position of every linear placed contig, the 64-bit scan (ig_kernels_rows.cuh) numbers
 * them, k_join_ends writes the table per contig (first position, positions, length in kb) and k_join_records one 16-byte record
 * per sub-fragment: (depth from the head, depth from the tail, run index or JOIN_UNPLACED / JOIN_RING, the position or 0: the
 * placement support, ig_kernels_place.cuh, reads the last).
 * The links: k_join_emit is the counting sort of the contacts in genome coordinates (k_lift_pass) with up to four emissions per
 * contact, entry = (row: the lower end, word: the upper end << 32 | count); the rows are sorted and the equal columns summed by
 * the kernels of ig_kernels_rows.cuh on this feature's own buffers.  Integer sums: the result does not depend on the launch
 * shapes or on the order in which the atomics land.
 * The model: k_join_model<G> over the links found, G lanes per link.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define JOIN_THREADS 256
#define JOIN_UNPLACED (-1)
#define JOIN_RING (-2)
#define JOIN_NS 7 /* the scalars the passes over the contacts own: the order of ig_join_support_build's scalars[0..5], then the entries */
#define JOIN_IN_REACH 0
#define JOIN_OUT_OF_REACH 1
#define JOIN_CIS 2
#define JOIN_RING_OBS 3
#define JOIN_UNPLACED_OBS 4
#define JOIN_CONTRIBUTIONS 5
#define JOIN_ENTRIES 6
#define JOIN_WAVE_PAIRS 66 /* links of more pairs (a full window of 11 positions has 66): a wave per link in the model pass, else a thread */

struct JoinEnd { /* per linear placed contig k */
    int start, n;
    float l_kb; /* (float) l_cont_bp / 1000.0f */
    int pad;
};

/* head[r] = 1 at the first position of a placed contig that is not a ring: the running sum less one is the run index k */
__global__ void __launch_bounds__(JOIN_THREADS) k_join_heads(const int2* __restrict__ meta, int T, unsigned long long* __restrict__ head)
{
    const int r = blockIdx.x * JOIN_THREADS + threadIdx.x;
    if (r >= T) return;
    const int2 m = meta[r];
    head[r] = (m.y > 0 && r == m.x) ? 1ull : 0ull;
}

/* the table of the contigs, written by their first positions.  LB: State.LB, the contig's length in bp on every bin */
__global__ void __launch_bounds__(JOIN_THREADS) k_join_ends(const int2* __restrict__ meta, const unsigned long long* __restrict__ incl, int T, int K,
                                                            const int* __restrict__ order, int M, const SubTab* __restrict__ sub,
                                                            const int* __restrict__ LB, int N, JoinEnd* __restrict__ ends)
{
    const int r = blockIdx.x * JOIN_THREADS + threadIdx.x;
    if (r >= T) return;
    const int2 m = meta[r];
    if (!(m.y > 0 && r == m.x)) return;
    const long long k = (long long)incl[r] - 1;
    if (k < 0 || k >= K) return;
    const int s = order[r];
    int bp = 0;
    if ((unsigned)s < (unsigned)M) {
        const int f = sub[s].parent;
        if ((unsigned)f < (unsigned)N) bp = LB[f];
    }
    ends[k] = JoinEnd{r, min(m.y, T - r), (float)bp / 1000.0f, 0};
}

/* one record per sub-fragment, one gather per contact endpoint (.w: the position of a placed sub-fragment, what the placement support reads) */
__global__ void __launch_bounds__(JOIN_THREADS) k_join_records(const int* __restrict__ pix, int M, int T, const int2* __restrict__ meta,
                                                               const unsigned long long* __restrict__ incl, int K, int4* __restrict__ rec)
{
    const int s = blockIdx.x * JOIN_THREADS + threadIdx.x;
    if (s >= M) return;
    const int p = pix[s];
    int4 out = make_int4(0, 0, JOIN_UNPLACED, 0);
    if (p >= 0 && p < T) {
        const int2 m = meta[p];
        const long long k = (long long)incl[p] - 1;
        if (m.y <= 0 || k < 0 || k >= K) out.z = JOIN_RING;
        else out = make_int4(p - m.x, m.x + m.y - 1 - p, (int)k, 0);
        out.w = p;
    }
    rec[s] = out;
}

/* One pass over the contacts (row of contact k: crow[k]; column and count: cc[k]), twice, shaped like k_lift_pass.
 * SCATTER = false: a trans contact between two linear placed contigs is tried against the four pairs of ends (sa, sb) in the order
 * (0, 0), (0, 1), (1, 0), (1, 1); where depth + depth + 1 <= window it counts for the row lo = min(end, end).  The classes of
 * contact, the contributions and the entries are summed in registers and reach memory once per workgroup.
 * SCATTER = true: the counters have become cursors; every emission takes the next slot of its row and writes (hi, count) there.
 * n_ent: the entries the first pass counted -- nothing is written beyond them.
 * COMBINE = false, the yardstick: one atomic per emission.  COMBINE = true: for each of the four emissions in turn a run of a
 * wave's lanes with an equal lo issues ONE atomic, by its head and for the run's length (rows_slot, ig_kernels_rows.cuh): late
 * in an assembly there are few ends, and every lane of a wave hits the same counter.
 * A sharded handle takes the rows i % world == rank. */
template <bool SCATTER, bool COMBINE>
__global__ void __launch_bounds__(JOIN_THREADS) k_join_emit(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                            const int4* __restrict__ rec, int window, int U, unsigned long long* __restrict__ counter,
                                                            unsigned long long* __restrict__ ent, unsigned long long n_ent,
                                                            unsigned long long* __restrict__ out_sc, int rank, int world)
{
    __shared__ unsigned long long sc[JOIN_NS];
    if (!SCATTER) class_zero<JOIN_NS>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_in = 0, r_out = 0, r_cis = 0, r_ring = 0, r_unpl = 0, r_contrib = 0, r_ent = 0;
    const long long stride = (long long)gridDim.x * JOIN_THREADS;
    const long long Zr = COMBINE ? (Z + 63) & ~63LL : Z; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * JOIN_THREADS + threadIdx.x; k < Zr; k += stride) {
        int da0 = 0, da1 = 0, db0 = 0, db1 = 0, ea = 0, eb = 0, cnt = 0;
        bool live = false; /* a trans contact between two linear placed contigs */
        if (k < Z) {
            const int i = crow[k];
            if (contact_is_mine(i, rank, world)) {
                const int2 e = cc[k];
                const int4 a = rec[i], b = rec[e.x];
                const unsigned long long cv = (unsigned long long)(long long)e.y;
                if (a.z == JOIN_UNPLACED || b.z == JOIN_UNPLACED) r_unpl += cv;
                else if (a.z < 0 || b.z < 0) r_ring += cv;
                else if (a.z == b.z) r_cis += cv;
                else if (2 * max(a.z, b.z) + 1 < U) { /* (always: the records and U are of one scan) */
                    live = true;
                    da0 = a.x, da1 = a.y, db0 = b.x, db1 = b.y;
                    ea = 2 * a.z, eb = 2 * b.z;
                    cnt = e.y;
                    const int n = (da0 + db0 < window) + (da0 + db1 < window) + (da1 + db0 < window) + (da1 + db1 < window);
                    if (!SCATTER) {
                        if (n) r_in += cv;
                        else r_out += cv;
                        r_contrib += cv * (unsigned long long)n;
                        r_ent += (unsigned long long)n;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int sa = q >> 1, sb = q & 1;
            int lo = -1, hi = 0; /* lo = -1: nothing to place */
            if (live && (sa ? da1 : da0) + (sb ? db1 : db0) < window) { /* depth + depth + 1 <= window */
                lo = min(ea + sa, eb + sb);
                hi = max(ea + sa, eb + sb);
            }
            unsigned long long slot = 0;
            if (!COMBINE) {
                if (lo >= 0) slot = atomicAdd(&counter[lo], 1ull);
            } else
                slot = rows_slot<SCATTER>(counter, lo, lane);
            if (SCATTER && lo >= 0 && slot < n_ent) ent[slot] = lift_pack(hi, cnt);
        }
    }
    if (SCATTER) return;
    if (r_in) atomicAdd(&sc[JOIN_IN_REACH], r_in);
    if (r_out) atomicAdd(&sc[JOIN_OUT_OF_REACH], r_out);
    if (r_cis) atomicAdd(&sc[JOIN_CIS], r_cis);
    if (r_ring) atomicAdd(&sc[JOIN_RING_OBS], r_ring);
    if (r_unpl) atomicAdd(&sc[JOIN_UNPLACED_OBS], r_unpl);
    if (r_contrib) atomicAdd(&sc[JOIN_CONTRIBUTIONS], r_contrib);
    if (r_ent) atomicAdd(&sc[JOIN_ENTRIES], r_ent);
    class_flush<JOIN_NS>(sc, out_sc);
}

/* pairs of a link between ends of contigs of na and nb positions: depth u = 0 .. ua - 1, ua = min(w, na), pairs with
 * min(nb, w - u) positions; the first r depths see all nb (join_support.pairs_closed_form) */
__device__ __forceinline__ long long join_pairs(int na, int nb, int w)
{
    const long long ua = min(w, na);
    const long long r = min(max((long long)w - nb + 1, 0ll), ua);
    return r * nb + (ua - r) * w - (ua - 1 + r) * (ua - r) / 2;
}

/* depth_kb of the position of depth u from end `side` of contig e: dist at the head, fabsf(L_kb - dist) at the tail */
__device__ __forceinline__ float join_depth_kb(const float* __restrict__ ds, const JoinEnd e, int side, int u)
{
    return side ? fabsf(e.l_kb - ds[e.start + e.n - 1 - u]) : ds[e.start + u];
}

/* The model part over the links found (row of link g: the last row that starts at or in front of g; its column: col[g]):
 * pairs[g] by the closed form, expected_q[g] = the sum of ig_quantize((double) ig_rippe(depth_kb + depth_kb, p)) under parameter set
 * 0 over the cells (u, v) of the rectangle min(w, na) x min(w, nb) with u + v + 1 <= w.
 * G lanes share a link: G = 64, a wave with an integer wave reduction, for the links of more than JOIN_WAVE_PAIRS pairs; G = 1, a
 * thread, for the others (behind a bomb a link has nine pairs).  Both launches walk every link and leave the other form's alone;
 * the sums are integer, so the choice cannot change the result.  *maxq takes the largest |q| seen (the host's overflow guard). */
template <int G>
__global__ void __launch_bounds__(JOIN_THREADS) k_join_model(const unsigned long long* __restrict__ rowptr, int U, const int* __restrict__ col,
                                                             long long n_links, const JoinEnd* __restrict__ ends, int K, const float* __restrict__ ds,
                                                             int T, int window, const Glob* __restrict__ g, unsigned long long* __restrict__ pairs,
                                                             unsigned long long* __restrict__ expected_q, unsigned long long* __restrict__ maxq)
{
    const long long link = ((long long)blockIdx.x * JOIN_THREADS + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    unsigned long long acc = 0, mx = 0;
    long long P = 0;
    bool mine = false;
    if (link < n_links) {
        int lo = 0, hi = U; /* the last row that starts at or in front of the link */
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rowptr[mid] <= (unsigned long long)link) lo = mid;
            else hi = mid;
        }
        const int eb = col[link];
        const int ka = lo >> 1, kb = eb >> 1;
        if (ka < K && kb >= 0 && kb < K) {
            const JoinEnd a = ends[ka], b = ends[kb];
            /* (a table that does not fit the positions: an inconsistent state -- nothing is read out of bounds) */
            if (a.start >= 0 && a.n > 0 && a.start + a.n <= T && b.start >= 0 && b.n > 0 && b.start + b.n <= T) {
                P = join_pairs(a.n, b.n, window);
                mine = G == 64 ? P > JOIN_WAVE_PAIRS : P <= JOIN_WAVE_PAIRS;
                if (mine) {
                    const ig_params p = g->par[0];
                    const int ua = min(window, a.n), vb = min(window, b.n);
                    const int cells = ua * vb; /* <= 1024 * 1024 */
                    for (int t = sub; t < cells; t += G) {
                        const int u = t / vb, v = t - u * vb;
                        if (u + v >= window) continue;
                        const float s = join_depth_kb(ds, a, lo & 1, u) + join_depth_kb(ds, b, eb & 1, v);
                        const long long q = ig_quantize((double)ig_rippe(s, p, ig_tab()));
                        acc += (unsigned long long)q;
                        const unsigned long long aq = (unsigned long long)(q < 0 ? -q : q);
                        mx = aq > mx ? aq : mx;
                    }
                }
            }
        }
    }
    /* (one loop for the maximum and the sum: their shuffles interleave; wave_max_u64 behind wave_sum_u64 measured slower) */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
        if (G == 64) acc += __shfl_xor(acc, d, 64);
    }
    if (mine && sub == 0) {
        pairs[link] = (unsigned long long)P;
        expected_q[link] = acc;
    }
    if ((threadIdx.x & 63) == 0) raise_max(maxq, mx);
}
