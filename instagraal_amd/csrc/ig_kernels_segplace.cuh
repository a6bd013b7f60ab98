/* ig_kernels_segplace.cuh -- segment placement support: where the contacts say a run of bins belongs, and which way round.  The
 * guests are the caller's SEGMENTS of the genome order (co-linear blocks, whole scaffolds, any intervals of positions inside one
 * contig); each gets its home, its best site and the runner-up as the placement support gives them for a bin
 * (ig_kernels_place.cuh), and at each of the three sites the four sums that say which way round the contacts would put it in.  The
 * rule is stated once, in instagraal_amd/segment_placement.py; the passes here reproduce its arrays byte for byte.
 *
 * The records: the join support's records (join_enqueue_records, ig_host_join.inc) give every sub-fragment its run index and its
 * position; k_segplace_map writes the segment of every position, k_segplace_records one record per segment in k_place_bins'
 * layout -- (first position g0, positions n_g, run or JOIN_RING, 0) -- and checks the caller's list.
 * The profile: k_segplace_emit is k_place_emit with the segment of an end for its bin, zero, one or two emissions per contact; the
 * rows are sorted and summed by the row builder, the 64-bit scan turns the summed counts into prefix sums.
 * The scan: k_place_scan<G>, unchanged, over the segment records.
 * The quadrants: k_segplace_windows turns the three sites of every segment into bounds in the original positions,
 * k_segplace_quadrants walks the contacts once more and adds every counted end that lies in an arm of its segment to the word of
 * (segment, site, arm, part of the window) it falls into: one 64-bit atomic per hit.
 *
 * Integer sums and the placement support's total order: the result does not depend on the launch shapes, on the form of the scan or
 * on the order in which the atomics land.  Nothing here writes anything a move reads. */
#pragma once

#define SEGPLACE_THREADS 256
#define SEGPLACE_NS 6 /* the scalars the passes over the contacts own: the order of ig_segment_placement's scalars[0..5] */
#define SEGPLACE_UNPLACED_OBS 0
#define SEGPLACE_RING_OBS 1
#define SEGPLACE_WITHIN_OBS 2
#define SEGPLACE_COUNTED_OBS 3
#define SEGPLACE_UNCOUNTED_OBS 4
#define SEGPLACE_ENTRIES 5
#define SEGPLACE_NI (PLACE_NI + 1) /* int32 arrays per segment: the placement support's, then the arm */
#define SEGPLACE_NL PLACE_NL       /* int64 arrays per segment */
#define SEGPLACE_SITES 3           /* home, best, second */
/* the quadrants: word (segment * 3 + site) * 4 + quadrant */
#define SEGPLACE_HL 0
#define SEGPLACE_HR 1
#define SEGPLACE_TL 2
#define SEGPLACE_TR 3

/* seg_of[r]: the segment position r lies in, -1: none -- one thread per position, a binary search over first[] (memory-safe whatever
 * the list holds: the host looks at the error word before anything reads seg_of) */
__global__ void __launch_bounds__(SEGPLACE_THREADS) k_segplace_map(const int* __restrict__ first, const int* __restrict__ last, int n_seg, int T,
                                                                   int* __restrict__ seg_of)
{
    const int r = blockIdx.x * SEGPLACE_THREADS + threadIdx.x;
    if (r >= T) return;
    int lo = 0, hi = n_seg; /* the segments in front of lo start at or before r */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    seg_of[r] = lo > 0 && last[lo - 1] >= r ? lo - 1 : -1;
}

/* One thread per segment k: the list is checked -- in range, ascending and disjoint (against the segment in front), both ends in one
 * contig by meta -- and a malformed one sets the error word (bit 0 range, 1 order, 2 two contigs): the host fails loudly.  recs[k] =
 * (g0, n_g, run or JOIN_RING, 0), the record k_place_scan reads for a bin; a segment of a malformed list gets (-1, 0, JOIN_RING, 0). */
__global__ void __launch_bounds__(SEGPLACE_THREADS) k_segplace_records(const int* __restrict__ first, const int* __restrict__ last, int n_seg,
                                                                       const int2* __restrict__ meta, const unsigned long long* __restrict__ incl, int T, int K,
                                                                       int4* __restrict__ recs, int* __restrict__ err_word)
{
    const int k = blockIdx.x * SEGPLACE_THREADS + threadIdx.x;
    if (k >= n_seg) return;
    const int f = first[k], l = last[k];
    int err = 0;
    if (f < 0 || l < f || l >= T) err |= 1;
    if (k > 0 && f <= last[k - 1]) err |= 2;
    int4 out = make_int4(-1, 0, JOIN_RING, 0);
    if (!err) {
        const int2 mf = meta[f], ml = meta[l];
        if (mf.x != ml.x) err |= 4;
        else {
            const long long run = (long long)incl[f] - 1;
            out = make_int4(f, l - f + 1, (mf.y > 0 && run >= 0 && run < K) ? (int)run : JOIN_RING, 0);
        }
    }
    recs[k] = out;
    if (err) atomicOr(err_word, err);
}

/* One pass over the contacts (row of contact k: crow[k]; column and count: cc[k]), twice, shaped like k_place_emit.
 * SCATTER = false: a contact is classified by the first class it fits (an end not placed, an end on a ring, both ends in one
 * segment, counted: an end in a segment, uncounted); a counted contact counts for the row of the segment of each end that has one.
 * The five class sums and the entries are summed in registers and reach memory once per workgroup.
 * SCATTER = true: the counters have become cursors; each emission takes the next slot of its row and writes (the position of the
 * other end, count) there.  n_ent: the entries the first pass counted -- nothing is written beyond them.
 * One atomic per emission. */
template <bool SCATTER>
__global__ void __launch_bounds__(SEGPLACE_THREADS) k_segplace_emit(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                                    const int4* __restrict__ rec, const int* __restrict__ seg_of, int T, int n_seg,
                                                                    unsigned long long* __restrict__ counter, unsigned long long* __restrict__ ent,
                                                                    unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[SEGPLACE_NS];
    if (!SCATTER) class_zero<SEGPLACE_NS>(sc);
    unsigned long long r_unpl = 0, r_ring = 0, r_within = 0, r_counted = 0, r_uncounted = 0, r_ent = 0;
    const long long stride = (long long)gridDim.x * SEGPLACE_THREADS;
    for (long long k = (long long)blockIdx.x * SEGPLACE_THREADS + threadIdx.x; k < Z; k += stride) {
        const int i = crow[k];
        const int2 e = cc[k];
        const int4 a = rec[i], b = rec[e.x];
        const unsigned long long cv = (unsigned long long)(long long)e.y;
        if (a.z == JOIN_UNPLACED || b.z == JOIN_UNPLACED) r_unpl += cv;
        else if (a.z < 0 || b.z < 0) r_ring += cv;
        else if ((unsigned)a.w < (unsigned)T && (unsigned)b.w < (unsigned)T) { /* (always: a placed record holds its position) */
            int sa = seg_of[a.w], sb = seg_of[b.w];
            if (sa >= n_seg) sa = -1; /* (never: nothing is counted out of bounds) */
            if (sb >= n_seg) sb = -1;
            if (sa >= 0 && sa == sb) r_within += cv;
            else if (sa < 0 && sb < 0) r_uncounted += cv;
            else if (!SCATTER) {
                r_counted += cv;
                if (sa >= 0) {
                    r_ent += 1ull;
                    atomicAdd(&counter[sa], 1ull);
                }
                if (sb >= 0) {
                    r_ent += 1ull;
                    atomicAdd(&counter[sb], 1ull);
                }
            } else {
                if (sa >= 0) {
                    const unsigned long long slot = atomicAdd(&counter[sa], 1ull);
                    if (slot < n_ent) ent[slot] = lift_pack(b.w, e.y);
                }
                if (sb >= 0) {
                    const unsigned long long slot = atomicAdd(&counter[sb], 1ull);
                    if (slot < n_ent) ent[slot] = lift_pack(a.w, e.y);
                }
            }
        }
    }
    if (SCATTER) return;
    if (r_unpl) atomicAdd(&sc[SEGPLACE_UNPLACED_OBS], r_unpl);
    if (r_ring) atomicAdd(&sc[SEGPLACE_RING_OBS], r_ring);
    if (r_within) atomicAdd(&sc[SEGPLACE_WITHIN_OBS], r_within);
    if (r_counted) atomicAdd(&sc[SEGPLACE_COUNTED_OBS], r_counted);
    if (r_uncounted) atomicAdd(&sc[SEGPLACE_UNCOUNTED_OBS], r_uncounted);
    if (r_ent) atomicAdd(&sc[SEGPLACE_ENTRIES], r_ent);
    class_flush<SEGPLACE_NS>(sc, out_sc);
}

/* One thread per segment s, behind the scan: the three sites k_place_scan wrote (out_i: its arrays, n_seg words each) as bounds in
 * the ORIGINAL positions, win[3 s + site] = (lo, mid, hi, 0): the left part of the site's window is lo <= q < mid, the right part
 * mid <= q < hi (place_bound: the shift to the guest's reduced order is monotone; a guest's own positions never hold the other end
 * of an entry of its row, so that is the whole test, at home too).  A site that does not exist gets (0, 0, 0, 0).  ends: the table of
 * the linear contigs by run index.  The arm of the guest, m = min(n_g / 2, w), goes to arm[s] (0: no guest). */
__global__ void __launch_bounds__(SEGPLACE_THREADS) k_segplace_windows(const int4* __restrict__ recs, int n_seg, const int* __restrict__ out_i,
                                                                       const JoinEnd* __restrict__ ends, int K, int T, int window, int4* __restrict__ win,
                                                                       int* __restrict__ arm)
{
    const int s = blockIdx.x * SEGPLACE_THREADS + threadIdx.x;
    if (s >= n_seg) return;
    const size_t n = (size_t)n_seg;
    const bool guest = out_i[s] == 0;
    PlaceRow r;
    r.col = nullptr, r.pre = nullptr, r.e0 = r.e1 = 0;
    r.g0 = recs[s].x, r.ng = out_i[3 * n + s], r.kg = out_i[n + s], r.ug = out_i[2 * n + s];
    r.w = window, r.mh = 1;
    const int m = guest ? min(r.ng / 2, window) : 0;
#pragma unroll
    for (int site = 0; site < SEGPLACE_SITES; site++) {
        const int k = site == 0 ? r.kg : out_i[(size_t)(3 * site + 2) * n + s], u = site == 0 ? r.ug : out_i[(size_t)(3 * site + 3) * n + s];
        int4 b = make_int4(0, 0, 0, 0);
        if (guest && k >= 0 && k < K) {
            const JoinEnd e = ends[k];
            const int np = e.n - (k == r.kg ? r.ng : 0);
            if (np >= 0 && u >= 0 && u <= np) {
                const int lo = max(0, u - window), hi = min(np, u + window);
                b = make_int4(place_bound(r, k, e.start, lo), place_bound(r, k, e.start, u), place_bound(r, k, e.start, hi), 0);
            }
        }
        win[3 * (size_t)s + site] = b;
    }
    arm[s] = m;
}

/* The quadrants: one pass over the contacts, the classes of k_segplace_emit.  For each end of a counted contact whose segment is a
 * guest and whose own position lies in the head arm [g0, g0 + m - 1] or the tail arm [g1 - m + 1, g1], and for each of the three
 * sites whose window holds the other end, the count goes to quad[(segment * 3 + site) * 4 + (HL, HR, TL, TR)] with one 64-bit
 * atomic.  recs: (g0, n_g, run, 0); win: k_segplace_windows' bounds (all zero for a segment that is no guest).  Contact-parallel,
 * grid-stride. */
__device__ __forceinline__ void segplace_end(int s, int own, int other, unsigned long long cv, int window, const int4* __restrict__ recs,
                                             const int4* __restrict__ win, unsigned long long* __restrict__ quad)
{
    const int4 g = recs[s];
    const int m = min(g.y / 2, window);
    int q;
    if (own < g.x + m) q = SEGPLACE_HL;
    else if (own > g.x + g.y - 1 - m) q = SEGPLACE_TL;
    else return; /* interior (m = 0: every position is) */
#pragma unroll
    for (int site = 0; site < SEGPLACE_SITES; site++) {
        const int4 b = win[3 * (size_t)s + site];
        if (other >= b.x && other < b.z) atomicAdd(&quad[(3 * (size_t)s + site) * 4 + q + (other >= b.y ? 1 : 0)], cv);
    }
}

__global__ void __launch_bounds__(SEGPLACE_THREADS) k_segplace_quadrants(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                                         const int4* __restrict__ rec, const int* __restrict__ seg_of, int T, int n_seg,
                                                                         int window, const int4* __restrict__ recs, const int4* __restrict__ win,
                                                                         unsigned long long* __restrict__ quad)
{
    const long long stride = (long long)gridDim.x * SEGPLACE_THREADS;
    for (long long k = (long long)blockIdx.x * SEGPLACE_THREADS + threadIdx.x; k < Z; k += stride) {
        const int i = crow[k];
        const int2 e = cc[k];
        const int4 a = rec[i], b = rec[e.x];
        if (a.z < 0 || b.z < 0) continue; /* an end not placed or on a ring */
        if ((unsigned)a.w >= (unsigned)T || (unsigned)b.w >= (unsigned)T) continue;
        int sa = seg_of[a.w], sb = seg_of[b.w];
        if (sa >= n_seg) sa = -1;
        if (sb >= n_seg) sb = -1;
        if (sa == sb) continue; /* within a segment, or both ends outside every segment */
        const unsigned long long cv = (unsigned long long)(long long)e.y;
        if (sa >= 0) segplace_end(sa, a.w, b.w, cv, window, recs, win, quad);
        if (sb >= 0) segplace_end(sb, b.w, a.w, cv, window, recs, win, quad);
    }
}
