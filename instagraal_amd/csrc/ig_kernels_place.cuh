/* ig_kernels_place.cuh -- placement support: where the contacts say each bin belongs.  For every GUEST (a placed bin of a linear
 * contig) the density of its contacts with the flanks it has now (home) against the densest window it would have at any other site
 * of any linear placed contig, and the runner-up.  The rule is stated once, in instagraal_amd/placement_support.py; the passes here
 * reproduce its arrays byte for byte.
 *
 * The records: the join support's heads, ends and records (join_enqueue_records, ig_host_join.inc) give every sub-fragment its run
 * index and its position; k_place_bins writes one record per bin: (first position g0, positions n_g, run or JOIN_UNPLACED /
 * JOIN_RING, 0).
 * The profile: k_place_emit is the counting sort of k_join_emit with two emissions per counted contact, entry = (row: the bin of
 * one end, word: the ORIGINAL position of the other end << 32 | count); the rows are sorted and the equal columns summed by the
 * kernels of ig_kernels_rows.cuh on this feature's own buffers, and the 64-bit scan there turns the summed counts
 * into exclusive prefix sums: a window sum is two binary searches and one subtraction.
 * The scan: k_place_scan<G>, the segmented sliding-window pass over the sorted sparse rows.  The shift from the original positions
 * to the guest's reduced order is monotone and is applied here (place_bound).  Not every site is visited: only the ends of the
 * stretches on which the density is monotone (placement_support.candidate_sites: four sites per entry, at most ten per touched
 * contig).  Integer sums and an integer comparison with a total order: the result does not depend on the launch shapes, on the
 * form of the scan or on the order in which the atomics land.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define PLACE_THREADS 256
#define PLACE_NS 5 /* the scalars the passes over the contacts own: the order of ig_placement_support's scalars[0..4] */
#define PLACE_UNPLACED_OBS 0
#define PLACE_RING_OBS 1
#define PLACE_WITHIN_OBS 2
#define PLACE_COUNTED_OBS 3
#define PLACE_ENTRIES 4
/* rows of more summed entries get a wave in the scan, the others a thread.  Not measured: at this value a lane of the wave form has
 * at least two entries of its own; the thread form is the yardstick (tools/placement_support_bench.py) */
#define PLACE_WAVE_ENTRIES 128
#define PLACE_NI 11 /* int32 arrays per bin, the order of placement_support.INT_ARRAYS */
#define PLACE_NL 6  /* int64 arrays per bin, the order of placement_support.LONG_ARRAYS */

/* one record per bin: (g0, n_g, run, 0).  A bin's sub-fragments have consecutive ids (State.sub_first, State.sl) and consecutive
 * positions, ascending or descending with its orientation.  rec: the join support's records, rec.w = the position. */
__global__ void __launch_bounds__(PLACE_THREADS) k_place_bins(const int* __restrict__ sub_first, const int* __restrict__ sl, int N, int M,
                                                              const int4* __restrict__ rec, int T, int4* __restrict__ bins)
{
    const int f = blockIdx.x * PLACE_THREADS + threadIdx.x;
    if (f >= N) return;
    const int s0 = sub_first[f], n = sl[f];
    int4 out = make_int4(-1, 0, JOIN_UNPLACED, 0);
    if (s0 >= 0 && n > 0 && n <= M - s0) {
        const int4 a = rec[s0], b = rec[s0 + n - 1];
        out.z = a.z;
        if (a.z >= 0) {
            const int g0 = min(a.w, b.w);
            /* (a bin whose ends are not n - 1 positions apart, or that leaves the order: an inconsistent state -- it is no guest) */
            if (b.z == a.z && max(a.w, b.w) - g0 == n - 1 && g0 >= 0 && n <= T - g0) out = make_int4(g0, n, a.z, 0);
            else out.z = JOIN_UNPLACED;
        }
    }
    bins[f] = out;
}

/* One pass over the contacts (row of contact k: crow[k]; column and count: cc[k]), twice, shaped like k_join_emit.
 * SCATTER = false: a contact is classified by the first class it fits (an end not placed, an end on a ring, both ends in one bin,
 * counted); a counted contact counts for the rows of both bins.  The four class sums and the entries are summed in registers and
 * reach memory once per workgroup.
 * SCATTER = true: the counters have become cursors; each of the two emissions takes the next slot of its row and writes (the
 * position of the other end, count) there.  n_ent: the entries the first pass counted -- nothing is written beyond them.
 * One atomic per emission. */
template <bool SCATTER>
__global__ void __launch_bounds__(PLACE_THREADS) k_place_emit(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                              const int4* __restrict__ rec, const SubTab* __restrict__ sub, int N,
                                                              unsigned long long* __restrict__ counter, unsigned long long* __restrict__ ent,
                                                              unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[PLACE_NS];
    if (!SCATTER) class_zero<PLACE_NS>(sc);
    unsigned long long r_unpl = 0, r_ring = 0, r_within = 0, r_counted = 0, r_ent = 0;
    const long long stride = (long long)gridDim.x * PLACE_THREADS;
    for (long long k = (long long)blockIdx.x * PLACE_THREADS + threadIdx.x; k < Z; k += stride) {
        const int i = crow[k];
        const int2 e = cc[k];
        const int4 a = rec[i], b = rec[e.x];
        const unsigned long long cv = (unsigned long long)(long long)e.y;
        if (a.z == JOIN_UNPLACED || b.z == JOIN_UNPLACED) r_unpl += cv;
        else if (a.z < 0 || b.z < 0) r_ring += cv;
        else {
            const int fa = sub[i].parent, fb = sub[e.x].parent;
            if (fa == fb) r_within += cv;
            else if ((unsigned)fa < (unsigned)N && (unsigned)fb < (unsigned)N) { /* (always: the table's parents are bins) */
                if (!SCATTER) {
                    r_counted += cv;
                    r_ent += 2ull;
                    atomicAdd(&counter[fa], 1ull);
                    atomicAdd(&counter[fb], 1ull);
                } else {
                    const unsigned long long sa = atomicAdd(&counter[fa], 1ull), sb = atomicAdd(&counter[fb], 1ull);
                    if (sa < n_ent) ent[sa] = lift_pack(b.w, e.y);
                    if (sb < n_ent) ent[sb] = lift_pack(a.w, e.y);
                }
            }
        }
    }
    if (SCATTER) return;
    if (r_unpl) atomicAdd(&sc[PLACE_UNPLACED_OBS], r_unpl);
    if (r_ring) atomicAdd(&sc[PLACE_RING_OBS], r_ring);
    if (r_within) atomicAdd(&sc[PLACE_WITHIN_OBS], r_within);
    if (r_counted) atomicAdd(&sc[PLACE_COUNTED_OBS], r_counted);
    if (r_ent) atomicAdd(&sc[PLACE_ENTRIES], r_ent);
    class_flush<PLACE_NS>(sc, out_sc);
}

/* a guest's row and what the rule needs of the guest */
struct PlaceRow {
    const int* col;                /* the positions of the row's entries, ascending; [e0, e1) */
    const unsigned long long* pre; /* pre[i]: the summed counts of the entries in front of entry i (of all rows) */
    long long e0, e1;
    int g0, ng, kg, ug; /* first position, positions, run, home offset */
    int w, mh;
};

struct PlaceSite {
    unsigned long long left, right; /* obs = left + right; 0: no site */
    int hosts, k, u;
};

/* first entry of the row at or behind position p */
__device__ __forceinline__ long long place_lower(const PlaceRow& r, int p)
{
    long long lo = r.e0, hi = r.e1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (r.col[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* the original position in front of which reduced offset v of contig k (first position s) begins: the guest's own positions lie
 * between the reduced offsets ug - 1 and ug, and its row has no entry on them */
__device__ __forceinline__ int place_bound(const PlaceRow& r, int k, int s, int v) { return s + v + ((k == r.kg && v > r.ug) ? r.ng : 0); }

/* the window of site (k, u) of a contig of np reduced positions, first position s */
__device__ __forceinline__ PlaceSite place_site(const PlaceRow& r, int k, int s, int np, int u)
{
    const int lo = max(0, u - r.w), hi = min(np, u + r.w);
    const unsigned long long a = r.pre[place_lower(r, place_bound(r, k, s, lo))], m = r.pre[place_lower(r, place_bound(r, k, s, u))],
                             b = r.pre[place_lower(r, place_bound(r, k, s, hi))];
    return PlaceSite{m - a, b - m, hi - lo, k, u};
}

/* x beats y: denser by exact integers (obs * hosts < 2^62: the host's overflow guard), on equality the lower (k, u) */
__device__ __forceinline__ bool place_beats(const PlaceSite& x, const PlaceSite& y)
{
    const unsigned long long ox = x.left + x.right, oy = y.left + y.right;
    if (ox == 0) return false;
    if (oy == 0) return true;
    const unsigned long long l = ox * (unsigned long long)y.hosts, q = oy * (unsigned long long)x.hosts;
    if (l != q) return l > q;
    return x.k != y.k ? x.k < y.k : x.u < y.u;
}

/* site (k, u) tried against the best so far: eligible (hosts, the home exclusion, the runner-up's exclusion around (xk, xu); xk = -1:
 * none) and with a contact */
__device__ __forceinline__ void place_try(const PlaceRow& r, int k, int s, int np, int u, int xk, int xu, PlaceSite& best)
{
    if (u < 0 || u > np) return;
    if (k == r.kg && abs(u - r.ug) < 2 * r.w) return;
    if (k == xk && abs(u - xu) < 2 * r.w) return;
    if (min(np, u + r.w) - max(0, u - r.w) < r.mh) return;
    const PlaceSite x = place_site(r, k, s, np, u);
    if (place_beats(x, best)) best = x;
}

/* the candidate sites entry e of the row stands for (placement_support.candidate_sites): the four around its two events, and, for the
 * first entry of its contig in the row, the contig's own: the ends, the kinks of hosts(u), the ends of {hosts >= min_hosts} and of
 * the exclusion zones */
__device__ __forceinline__ void place_entry(const PlaceRow& r, long long e, const int2* __restrict__ meta, const unsigned long long* __restrict__ incl,
                                            int T, int K, int xk, int xu, PlaceSite& best)
{
    const int p = r.col[e];
    if (p < 0 || p >= T) return;
    const int2 m = meta[p];
    const long long kk = (long long)incl[p] - 1;
    if (m.y <= 0 || m.x < 0 || p < m.x || m.y > T - m.x || p - m.x >= m.y || kk < 0 || kk >= K) return; /* (an inconsistent state: nothing is read out of bounds) */
    const int k = (int)kk, s = m.x;
    const bool own = k == r.kg;
    const int np = m.y - (own ? r.ng : 0);
    const int o = p - s, x = o - ((own && o > r.ug) ? r.ng : 0);
    if (np <= 0 || x < 0 || x >= np) return;
    place_try(r, k, s, np, x - r.w, xk, xu, best);
    place_try(r, k, s, np, x - r.w + 1, xk, xu, best);
    place_try(r, k, s, np, x + r.w, xk, xu, best);
    place_try(r, k, s, np, x + r.w + 1, xk, xu, best);
    if (e > r.e0 && r.col[e - 1] >= s) return; /* not the first entry of its contig */
    const int ua = max(0, r.mh - r.w);
    place_try(r, k, s, np, 0, xk, xu, best);
    place_try(r, k, s, np, np, xk, xu, best);
    place_try(r, k, s, np, r.w, xk, xu, best);
    place_try(r, k, s, np, np - r.w, xk, xu, best);
    place_try(r, k, s, np, ua, xk, xu, best);
    place_try(r, k, s, np, np - ua, xk, xu, best);
    if (own) {
        place_try(r, k, s, np, r.ug - 2 * r.w, xk, xu, best);
        place_try(r, k, s, np, r.ug + 2 * r.w, xk, xu, best);
    }
    if (k == xk) {
        place_try(r, k, s, np, xu - 2 * r.w, xk, xu, best);
        place_try(r, k, s, np, xu + 2 * r.w, xk, xu, best);
    }
}

/* the maximum of a wave's sites under place_beats: a total order, so every lane ends with the same site */
__device__ __forceinline__ PlaceSite place_wave_max(PlaceSite x)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        PlaceSite y;
        y.left = __shfl_xor(x.left, d, 64);
        y.right = __shfl_xor(x.right, d, 64);
        y.hosts = __shfl_xor(x.hosts, d, 64);
        y.k = __shfl_xor(x.k, d, 64);
        y.u = __shfl_xor(x.u, d, 64);
        if (place_beats(y, x)) x = y;
    }
    return x;
}

/* the best eligible site of the row with a contact (obs = 0: none), less the zone of 2 w sites around (xk, xu) (xk = -1: no zone) */
template <int G>
__device__ __forceinline__ PlaceSite place_best(const PlaceRow& r, int sub, const int2* __restrict__ meta, const unsigned long long* __restrict__ incl, int T,
                                                int K, int xk, int xu)
{
    PlaceSite best{0ull, 0ull, 0, -1, 0};
    for (long long e = r.e0 + sub; e < r.e1; e += G) place_entry(r, e, meta, incl, T, K, xk, xu, best);
    return G == 64 ? place_wave_max(best) : best;
}

/* The scan: G lanes share a row (a bin).  G = 64, a wave that deals the row's entries out to its lanes and takes an integer wave
 * maximum, for the rows of more than wave_entries summed entries; G = 1, a thread, for the others.  Both launches walk every row and
 * leave the other form's alone (wave_entries < 0: every row is the wave's; beyond every row: the thread's).  Home, then the best site,
 * then the runner-up: the same pass with one more exclusion zone.  out_i: PLACE_NI arrays of N int32, out_l: PLACE_NL arrays of N
 * int64, in the order of placement_support.INT_ARRAYS / LONG_ARRAYS. */
template <int G>
__global__ void __launch_bounds__(PLACE_THREADS) k_place_scan(const int4* __restrict__ bins, int N, const unsigned long long* __restrict__ rowptr,
                                                              const int* __restrict__ col, const unsigned long long* __restrict__ pre, long long n_ent,
                                                              const int2* __restrict__ meta, const unsigned long long* __restrict__ incl, int T, int K,
                                                              int window, int min_hosts, long long wave_entries, int* __restrict__ out_i,
                                                              long long* __restrict__ out_l)
{
    const long long f = ((long long)blockIdx.x * PLACE_THREADS + threadIdx.x) / G;
    const int sub = threadIdx.x % G;
    if (f >= N) return; /* (G = 64: a whole wave leaves together) */
    const int4 b = bins[f];
    PlaceRow r;
    r.col = col;
    r.pre = pre;
    r.e1 = (long long)min(rowptr[f + 1], (unsigned long long)n_ent);
    r.e0 = min((long long)rowptr[f], r.e1);
    const bool mine = G == 64 ? r.e1 - r.e0 > wave_entries : r.e1 - r.e0 <= wave_entries;
    if (!mine) return;
    bool guest = b.z >= 0 && b.z < K && b.x >= 0 && b.y > 0 && b.y <= T - b.x;
    int2 hm = make_int2(0, 0);
    if (guest) { /* (a record that does not fit its contig: an inconsistent state -- no guest, nothing is read out of bounds) */
        hm = meta[b.x];
        guest = hm.y > 0 && hm.x >= 0 && hm.x <= b.x && hm.y <= T - hm.x && b.y <= hm.x + hm.y - b.x;
    }
    PlaceSite home{0ull, 0ull, 0, -1, 0}, s1 = home, s2 = home;
    int n_g = 0;
    if (guest) {
        r.g0 = b.x, r.ng = b.y, r.kg = b.z, r.ug = b.x - hm.x;
        r.w = window, r.mh = min_hosts;
        n_g = b.y;
        home = place_site(r, r.kg, hm.x, hm.y - r.ng, r.ug);
        s1 = place_best<G>(r, sub, meta, incl, T, K, -1, 0);
        if (s1.left + s1.right != 0) s2 = place_best<G>(r, sub, meta, incl, T, K, s1.k, s1.u);
    }
    if (sub != 0) return;
    const size_t n = (size_t)N;
    out_i[f] = guest ? 0 : (b.z == JOIN_RING ? 2 : 1);
    out_i[n + f] = home.k;
    out_i[2 * n + f] = home.u;
    out_i[3 * n + f] = n_g;
    out_i[4 * n + f] = home.hosts;
    out_i[5 * n + f] = s1.k;
    out_i[6 * n + f] = s1.u;
    out_i[7 * n + f] = s1.hosts;
    out_i[8 * n + f] = s2.k;
    out_i[9 * n + f] = s2.u;
    out_i[10 * n + f] = s2.hosts;
    out_l[f] = (long long)home.left;
    out_l[n + f] = (long long)home.right;
    out_l[2 * n + f] = (long long)s1.left;
    out_l[3 * n + f] = (long long)s1.right;
    out_l[4 * n + f] = (long long)s2.left;
    out_l[5 * n + f] = (long long)s2.right;
}
