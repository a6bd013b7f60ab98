/* ig_kernels_pre.cuh -- the input folder from an assembly FASTA and read pairs: the restriction digest of the
 * records, G+C per fragment, and the fragment of every pair end, from which the row builder makes the pixels.  The rule is stated
 * once, in instagraal_amd/pre.py; the passes here reproduce its arrays byte for byte.
 *
 * The records lie one behind the other in ONE coordinate, a zero byte (the separator) behind each.  A base becomes a code: one bit per
 * plain letter A, C, G, T and the "valid letter" bit (an ambiguity code has that bit alone, a separator none); a site letter is the
 * mask of the bits it accepts, N the valid bit -- so no match reaches across a separator, and no thread asks which record it is in.
 * A cut is a bit in a bitmap over the coordinate; a record's first slot (the cut 0) and its separator (the cut at its length) are set
 * too, so order and de-duplication come from the bitmap itself.
 *
 * Here: k_pre_sites (16 bases per thread plus a halo of 15, the cuts as atomic ORs, the G+C bits as a plain store), k_pre_marks (the
 * sentinels), k_pre_popc (both bitmaps' words counted for the shared 64-bit scan), k_pre_cuts (the compaction), k_pre_frags (the
 * fragment table and G+C as a difference of two prefix counts), k_pre_assign (the binary search of a pair end, the wave-aggregated
 * append to the store) and k_pre_emit (the emit kernel of the row builder).
 *
 * Nothing here reads or writes anything a move reads or writes. */
#pragma once

#define PRE_THREADS 256
#define PRE_RUN 16         /* bases a thread of k_pre_sites owns: one 16-byte load (and one more for the halo) */
#define PRE_MAX_SITE 16    /* pre.MAX_SITE: the halo is PRE_MAX_SITE - 1 bases at the most, the cut of a match at most PRE_MAX_SITE behind it */
#define PRE_MAX_ENZYMES 4  /* pre.MAX_ENZYMES */
#define PRE_BIT_A 1
#define PRE_BIT_C 2
#define PRE_BIT_G 4
#define PRE_BIT_T 8
#define PRE_BIT_VALID 16
/* the letters ABCDGHKMNRSTVWY, a bit per letter of the alphabet (a = bit 0) */
#define PRE_LETTERS ((1u << 0) | (1u << 1) | (1u << 2) | (1u << 3) | (1u << 6) | (1u << 7) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 17) | (1u << 18) | (1u << 19) | (1u << 21) | (1u << 22) | (1u << 24))
#define PRE_NS 5 /* the scalars k_pre_assign sums: pre.SCALARS[0..4] */
#define PRE_IN 0
#define PRE_KEPT 1
#define PRE_MISS1 2
#define PRE_MISS2 3
#define PRE_BEYOND 4

/* the enzymes of one digest: wave-uniform, passed by value */
struct PreSites {
    int n;
    int len[PRE_MAX_ENZYMES], cut[PRE_MAX_ENZYMES];
    unsigned char mask[PRE_MAX_ENZYMES][PRE_MAX_SITE];
};

/* a byte of either case -> its code (pre.CODE) */
__device__ __forceinline__ unsigned pre_code(unsigned b)
{
    const unsigned i = (b & 0x1fu) - 1u; /* the letter's place in the alphabet where b is a letter */
    if ((b & 0xc0u) != 0x40u || i >= 26u || !((PRE_LETTERS >> i) & 1u)) return 0u;
    return PRE_BIT_VALID | (i == 0u ? PRE_BIT_A : 0u) | (i == 2u ? PRE_BIT_C : 0u) | (i == 6u ? PRE_BIT_G : 0u) | (i == 19u ? PRE_BIT_T : 0u);
}

/* Run t: the bases 16 t .. 16 t + 15 and the 16 behind them (seq is padded with zero bytes to 16 (n_runs + 1)).  The 32 codes
 * become five 32-bit planes, a bit per base; a site letter's plane is the OR of the planes its mask names, and the starts that match
 * are the AND of the letters' planes, each shifted by its place.  cutbits: 64-bit words over the coordinate, bit x & 63 of word
 * x >> 6; a run is a quarter of a word and its cuts reach at most 16 bits into the next quarter.  gcbits: the same bitmap as 16-bit
 * words, one per run. */
__global__ void __launch_bounds__(PRE_THREADS) k_pre_sites(const unsigned char* __restrict__ seq, long long n_runs, PreSites sites,
                                                           unsigned long long* __restrict__ cutbits, unsigned short* __restrict__ gcbits)
{
    const long long stride = (long long)gridDim.x * PRE_THREADS;
    for (long long t = (long long)blockIdx.x * PRE_THREADS + threadIdx.x; t < n_runs; t += stride) {
        const uint4 a = ((const uint4*)seq)[t], b = ((const uint4*)seq)[t + 1];
        const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        unsigned plane[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < 32; p++) {
            const unsigned code = pre_code((w[p >> 2] >> ((p & 3) * 8)) & 0xffu);
#pragma unroll
            for (int k = 0; k < 5; k++) plane[k] |= ((code >> k) & 1u) << p;
        }
        unsigned cuts = 0u;
        for (int e = 0; e < sites.n; e++) {
            unsigned match = 0xffffu;
            for (int j = 0; j < sites.len[e]; j++) {
                const unsigned m = sites.mask[e][j];
                unsigned accept = 0u;
#pragma unroll
                for (int k = 0; k < 5; k++)
                    if ((m >> k) & 1u) accept |= plane[k];
                match &= accept >> j;
            }
            cuts |= match << sites.cut[e]; /* 16 starts, a cut at most 16 behind its start: 32 bits */
        }
        if (cuts) {
            const int sh = (int)(t & 3) * 16;
            const unsigned long long lo = (unsigned long long)cuts << sh;
            const unsigned long long hi = sh > 32 ? (unsigned long long)(cuts >> (64 - sh)) : 0ull;
            if (lo) atomicOr(&cutbits[t >> 2], lo);
            if (hi) atomicOr(&cutbits[(t >> 2) + 1], hi);
        }
        gcbits[t] = (unsigned short)((plane[1] | plane[2]) & 0xffffu);
    }
}

/* the sentinels of every record: its first slot and its separator */
__global__ void __launch_bounds__(PRE_THREADS) k_pre_marks(const long long* __restrict__ off, const int* __restrict__ len, int R,
                                                           unsigned long long* __restrict__ cutbits)
{
    const int r = blockIdx.x * PRE_THREADS + threadIdx.x;
    if (r >= R) return;
    const long long a = off[r], b = a + len[r];
    atomicOr(&cutbits[a >> 6], 1ull << (a & 63));
    atomicOr(&cutbits[b >> 6], 1ull << (b & 63));
}

/* cnt[0][W]: the cuts of every word, cnt[1][W]: its G and C */
__global__ void __launch_bounds__(PRE_THREADS) k_pre_popc(const unsigned long long* __restrict__ cutbits, const unsigned long long* __restrict__ gcbits,
                                                          long long W, unsigned long long* __restrict__ cnt)
{
    const long long stride = (long long)gridDim.x * PRE_THREADS;
    for (long long w = (long long)blockIdx.x * PRE_THREADS + threadIdx.x; w < W; w += stride) {
        cnt[w] = (unsigned long long)__popcll(cutbits[w]);
        cnt[W + w] = (unsigned long long)__popcll(gcbits[w]);
    }
}

/* the set bits in order: cuts[rank] = coordinate.  incl: the inclusive prefix sums of cnt[0] */
__global__ void __launch_bounds__(PRE_THREADS) k_pre_cuts(const unsigned long long* __restrict__ cutbits, const unsigned long long* __restrict__ incl,
                                                          long long W, long long* __restrict__ cuts, long long n_cuts)
{
    const long long stride = (long long)gridDim.x * PRE_THREADS;
    for (long long w = (long long)blockIdx.x * PRE_THREADS + threadIdx.x; w < W; w += stride) {
        unsigned long long bits = cutbits[w];
        if (!bits) continue;
        long long rank = (long long)incl[w] - __popcll(bits);
        while (bits) {
            const int b = __ffsll((long long)bits) - 1;
            bits &= bits - 1;
            if (rank >= 0 && rank < n_cuts) cuts[rank] = w * 64 + b;
            rank++;
        }
    }
}

/* G and C in front of coordinate x.  gcincl: the inclusive prefix sums of cnt[1] */
__device__ __forceinline__ long long pre_gc_before(const unsigned long long* __restrict__ gcbits, const unsigned long long* __restrict__ gcincl, long long x)
{
    const long long w = x >> 6;
    return (w ? (long long)gcincl[w - 1] : 0ll) + __popcll(gcbits[w] & ((1ull << (x & 63)) - 1ull));
}

/* One cut per thread.  Cut g at coordinate x lies in record r (the last whose offset is <= x); the records in front of it own one
 * sentinel more than fragments each, so a cut that is no separator starts the global fragment g - r, which ends at the next cut. */
__global__ void __launch_bounds__(PRE_THREADS) k_pre_frags(const long long* __restrict__ cuts, long long n_cuts, const long long* __restrict__ off,
                                                           const int* __restrict__ len, int R, const unsigned long long* __restrict__ gcbits,
                                                           const unsigned long long* __restrict__ gcincl, long long n_frags, long long* __restrict__ rec_first,
                                                           int* __restrict__ frag_rec, int* __restrict__ start, int* __restrict__ end, int* __restrict__ gc)
{
    const long long stride = (long long)gridDim.x * PRE_THREADS;
    for (long long g = (long long)blockIdx.x * PRE_THREADS + threadIdx.x; g < n_cuts; g += stride) {
        const long long x = cuts[g];
        int lo = 0, hi = R; /* the first record whose offset is beyond x lies in [lo, hi] */
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        const int r = lo - 1;
        if (r < 0) continue;
        const long long o = off[r];
        if (x == o + len[r]) continue; /* the separator: the end of the record's last fragment */
        const long long f = g - r;
        if (f < 0 || f >= n_frags || g + 1 >= n_cuts) continue;
        const long long y = cuts[g + 1];
        if (x == o) rec_first[r] = f;
        frag_rec[f] = r;
        start[f] = (int)(x - o);
        end[f] = (int)(y - o);
        gc[f] = (int)(pre_gc_before(gcbits, gcincl, y) - pre_gc_before(gcbits, gcincl, x));
    }
}

/* One end: record c, 1-based position p -> the global fragment, -1: none.  start[rec_first[c] .. rec_first[c + 1]) are the starts of
 * record c's fragments, ascending from 0: searchsorted(starts, p - 1, "right") - 1.  *beyond: p lies behind the record's end (it
 * falls into the last fragment all the same). */
__device__ __forceinline__ int pre_fragment_of(int c, int p, const long long* __restrict__ rec_first, const int* __restrict__ len, int R,
                                               const int* __restrict__ start, bool* beyond)
{
    *beyond = false;
    if (c < 0 || c >= R) return -1;
    *beyond = p > len[c];
    if (p < 1) return -1;
    const int pos0 = p - 1;
    long long lo = rec_first[c], hi = rec_first[c + 1];
    const long long first = lo;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (start[mid] <= pos0) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1 < first ? -1 : (int)(lo - 1);
}

/* One pair per thread; a kept pair is appended to the store behind *cursor as (min, max) of its two fragments: the kept lanes of a
 * wave are counted by a ballot, one lane draws their places with one atomic (as k_pairs_lift).  cap: the store's capacity -- nothing
 * is written beyond it. */
__global__ void __launch_bounds__(PRE_THREADS) k_pre_assign(const int* __restrict__ c1, const int* __restrict__ p1, const int* __restrict__ c2,
                                                            const int* __restrict__ p2, long long n, const long long* __restrict__ rec_first,
                                                            const int* __restrict__ len, int R, const int* __restrict__ start, int2* __restrict__ store,
                                                            unsigned long long* __restrict__ cursor, unsigned long long cap, unsigned long long* __restrict__ out_sc)
{
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * PRE_THREADS;
    const long long nr = (n + 63) & ~63LL; /* whole waves stay in the loop together (the ballots need every lane) */
    unsigned long long w_in = 0, w_kept = 0, w_m1 = 0, w_m2 = 0, w_bey = 0; /* per wave, the same in every lane */
    for (long long k = (long long)blockIdx.x * PRE_THREADS + threadIdx.x; k < nr; k += stride) {
        const bool live = k < n;
        int status = -1, fa = -1, fb = -1;
        bool ba = false, bb = false;
        if (live) {
            fa = pre_fragment_of(c1[k], p1[k], rec_first, len, R, start, &ba);
            fb = pre_fragment_of(c2[k], p2[k], rec_first, len, R, start, &bb);
            status = fa < 0 ? 1 : fb < 0 ? 2 : 0;
        }
        const unsigned long long kept = __ballot(status == 0);
        w_in += (unsigned long long)__popcll(__ballot(live));
        w_kept += (unsigned long long)__popcll(kept);
        w_m1 += (unsigned long long)__popcll(__ballot(status == 1));
        w_m2 += (unsigned long long)__popcll(__ballot(status == 2));
        w_bey += (unsigned long long)(__popcll(__ballot(ba)) + __popcll(__ballot(bb)));
        if (kept) { /* (the same in every lane) */
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(kept));
            base = __shfl(base, 0, 64);
            if (status == 0) {
                const unsigned long long slot = base + (unsigned long long)__popcll(kept & ((1ull << lane) - 1ull));
                if (slot < cap) store[slot] = make_int2(min(fa, fb), max(fa, fb));
            }
        }
    }
    if (lane == 0) {
        if (w_in) atomicAdd(&out_sc[PRE_IN], w_in);
        if (w_kept) atomicAdd(&out_sc[PRE_KEPT], w_kept);
        if (w_m1) atomicAdd(&out_sc[PRE_MISS1], w_m1);
        if (w_m2) atomicAdd(&out_sc[PRE_MISS2], w_m2);
        if (w_bey) atomicAdd(&out_sc[PRE_BEYOND], w_bey);
    }
}

/* The emit kernel of the pixels: one pass over the store, twice (the counting sort of the row builder).  A stored pair is an entry
 * (row min, word max << 32 | 1); out_sc[0]: the entries, out_sc[1]: pairs with a fragment outside 0 .. U - 1 (none: the host refuses
 * the build then). */
template <bool SCATTER>
__global__ void __launch_bounds__(PRE_THREADS) k_pre_emit(const int2* __restrict__ store, long long n, int U, unsigned long long* __restrict__ counter,
                                                          unsigned long long* __restrict__ ent, unsigned long long n_ent, unsigned long long* __restrict__ out_sc)
{
    __shared__ unsigned long long sc[2];
    if (!SCATTER) class_zero<2>(sc);
    const int lane = threadIdx.x & 63;
    unsigned long long r_ent = 0, r_bad = 0;
    const long long stride = (long long)gridDim.x * PRE_THREADS;
    const long long nr = (n + 63) & ~63LL;
    for (long long k = (long long)blockIdx.x * PRE_THREADS + threadIdx.x; k < nr; k += stride) {
        int lo = -1, hi = 0;
        if (k < n) {
            const int2 e = store[k];
            if (e.x < 0 || e.y < e.x || e.y >= U) r_bad++;
            else {
                lo = e.x;
                hi = e.y;
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
