/* ig_kernels_emap.cuh -- the expected contact map of the current genome: for every pixel pair of the contact map's image what the
 * model in use predicts of the sub-fragment pairs that fall into it.  The rule is stated once, in instagraal_amd/expected_map.py;
 * the kernels here reproduce it entry for entry.
 *
 * Three images of side x side 64-bit words in ig_contact_map's convention (k_map_mirror writes the lower half and doubles the
 * diagonal; the passes here fill the upper triangle [min][max] only): cis_q, the sum of
 * q(i, k) = ig_quantize((double) ig_rippe(fabsf(ds_i - ds_k), p)) under parameter set 0 over the pairs i < k of one placed contig
 * that is not a ring; cis_pairs, their number; ring_pairs, the number of pairs on a ring (no model value: a pair on a ring has two
 * separations).  Integer sums: the result does not depend on threads, waves, workgroups or the order of the atomics, and the two
 * forms below return the same bytes.  The positions, ds and meta are the contact map's and the distance law's (k_map_pixels,
 * k_law_sorted).  No contact is read: the result does not depend on the shard.
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define EMAP_THREADS 256
#define EMAP_WAVES (EMAP_THREADS / 64)
#define EMAP_NS 8 /* EmapBuf.sc, in 64-bit words */
#define EMAP_SC_LINEAR 0      /* pairs of the placed linear contigs */
#define EMAP_SC_RING 1        /* pairs of the placed rings */
#define EMAP_SC_MAXQ 2        /* the largest |quantised model value| seen */
#define EMAP_SC_TILES_EVAL 3  /* tile form: tiles whose pairs were walked */
#define EMAP_SC_TILES_CONST 4 /* tile form: tiles written as pairs x one value */
#define EMAP_SC_NONMONO 5     /* ds decreases somewhere inside a linear contig: the constant shortcut is not sound */

/* the model's log2 / exp2 table into the workgroup's LDS (ds_read instead of a global gather per evaluation) */
__device__ __forceinline__ void emap_load_tab(double* tab)
{
    const double* T = ig_tab();
    for (int i = threadIdx.x; i < IG_TAB_SIZE; i += EMAP_THREADS) tab[i] = T[i];
    __syncthreads();
}

/* what every pair at or beyond d_max gets: ig_rippe's clamp of 0 from below by v_inter */
__device__ __forceinline__ long long emap_q_far(const ig_params& p) { return ig_quantize((double)ig_fmaxf(0.0f, p.v_inter)); }

/* One thread per position r: the pairs it opens (the k behind it in its contig) summed into the two scalars, the monotony of ds at
 * r, and (cnt != nullptr: the tile form) where r is the last position of its pixel a the number of listed tiles of a: the pixels b
 * from a up to the pixel of the last position of r's contig -- contigs that end inside a pair with nothing beyond it. */
__global__ void __launch_bounds__(EMAP_THREADS) k_emap_count(const float* __restrict__ ds, const int2* __restrict__ meta, int T, int bin,
                                                             unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ sc)
{
    const int r = blockIdx.x * EMAP_THREADS + threadIdx.x;
    unsigned long long lin = 0, ring = 0;
    if (r < T) {
        const int2 m = meta[r];
        const bool is_ring = m.y < 0;
        const int start = max(m.x, 0);
        const int end = (int)min((long long)start + (is_ring ? -(long long)m.y : (long long)m.y), (long long)T);
        const unsigned long long behind = end - 1 > r ? (unsigned long long)(end - 1 - r) : 0ull;
        if (is_ring) ring = behind;
        else lin = behind;
        if (behind && !is_ring && ds[r + 1] < ds[r]) atomicOr(&sc[EMAP_SC_NONMONO], 1ull);
        if (cnt && (r == T - 1 || (r + 1) % bin == 0)) {
            const int a = r / bin;
            cnt[a] = (unsigned long long)(max(end - 1, r) / bin - a + 1);
        }
    }
    lin = wave_sum_u64(lin);
    ring = wave_sum_u64(ring);
    if ((threadIdx.x & 63) == 0) {
        if (lin) atomicAdd(&sc[EMAP_SC_LINEAR], lin);
        if (ring) atomicAdd(&sc[EMAP_SC_RING], ring);
    }
}

/* The row form, the yardstick: one thread per position r walks the k behind it in its contig, keeps the running sum and the pair
 * count while k stays in one pixel and issues one atomic per image at every change of pixel, on the cell [pixel of r][pixel of k]
 * (k > r: the upper triangle).  Rings only count. */
__global__ void __launch_bounds__(EMAP_THREADS) k_emap_rows(const float* __restrict__ ds, const int2* __restrict__ meta, int T, int bin, int side,
                                                            const Glob* __restrict__ g, unsigned long long* __restrict__ cis_q,
                                                            unsigned long long* __restrict__ cis_pairs, unsigned long long* __restrict__ ring_pairs,
                                                            unsigned long long* __restrict__ sc)
{
    __shared__ double tab[IG_TAB_SIZE];
    emap_load_tab(tab);
    const int r = blockIdx.x * EMAP_THREADS + threadIdx.x;
    const ig_params p = g->par[0];
    unsigned long long mx = 0;
    if (r < T) {
        const int2 m = meta[r];
        const bool is_ring = m.y < 0;
        const int start = max(m.x, 0);
        const int end = (int)min((long long)start + (is_ring ? -(long long)m.y : (long long)m.y), (long long)T);
        const size_t row = (size_t)(r / bin) * (size_t)side;
        const float dr = ds[r];
        int k = r + 1;
        while (k < end) {
            const int pb = k / bin;
            const int stop = (int)min(((long long)pb + 1) * bin, (long long)end);
            const unsigned long long n = (unsigned long long)(stop - k);
            if (is_ring) {
                atomicAdd(&ring_pairs[row + pb], n);
                k = stop;
                continue;
            }
            unsigned long long acc = 0;
            for (; k < stop; k++) {
                const long long q = ig_quantize((double)ig_rippe(fabsf(dr - ds[k]), p, tab));
                acc += (unsigned long long)q;
                const unsigned long long aq = (unsigned long long)(q < 0 ? -q : q);
                mx = aq > mx ? aq : mx;
            }
            atomicAdd(&cis_pairs[row + pb], n);
            if (acc) atomicAdd(&cis_q[row + pb], acc);
        }
    }
    mx = wave_max_u64(mx);
    if ((threadIdx.x & 63) == 0) raise_max(&sc[EMAP_SC_MAXQ], mx);
}

/* The work list of the tile form from the exclusive prefix sums off[0 .. side] of k_emap_count's counts: entry t is the tile
 * (a, a + t - off[a]) of the pixel a with off[a] <= t < off[a + 1]. */
__global__ void __launch_bounds__(EMAP_THREADS) k_emap_list(const unsigned long long* __restrict__ off, int side, long long n_tiles, int2* __restrict__ list)
{
    const long long t = (long long)blockIdx.x * EMAP_THREADS + threadIdx.x;
    if (t >= n_tiles) return;
    int lo = 0, hi = side; /* off[lo] <= t < off[hi] */
    while (lo + 1 < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= (unsigned long long)t) lo = mid;
        else hi = mid;
    }
    /* (counts that are not the list's -- an inconsistent table -- stay inside the image: the host compared n_tiles with the triangle) */
    list[t] = make_int2(lo, (int)min((long long)lo + (t - (long long)off[lo]), (long long)side - 1));
}

/* The tile form: one workgroup per listed tile (a, b), a <= b, evaluates the pairs i in pixel a, k in pixel b, k > i, of one
 * contig -- a pixel may straddle several -- reduces in integers, wave first and then through LDS, and STORES its three words: it
 * owns the cell.  Where the k of a row are at least a wave (bin >= 64) a wave takes a row of i and its lanes the k; below that the
 * pairs of the tile are dealt out one by one.
 *
 * SHORTCUT.  The cis pairs of a tile off the diagonal all belong to the contig of the last position of pixel a.  ds does not
 * decrease inside a linear contig (k_emap_count has checked it) and the f32 subtraction is monotone, so the smallest separation of
 * the tile is fabsf(ds[first k] - ds[last i]); where that is >= d_max the model gives every pair the same value (emap_q_far) and
 * the tile is pairs x that value, without an evaluation. */
template <bool SHORTCUT>
__global__ void __launch_bounds__(EMAP_THREADS) k_emap_tiles(const int2* __restrict__ list, const float* __restrict__ ds, const int2* __restrict__ meta, int T,
                                                             int bin, int side, const Glob* __restrict__ g, unsigned long long* __restrict__ cis_q,
                                                             unsigned long long* __restrict__ cis_pairs, unsigned long long* __restrict__ ring_pairs,
                                                             unsigned long long* __restrict__ sc)
{
    __shared__ double tab[IG_TAB_SIZE];
    __shared__ unsigned long long red[EMAP_WAVES][4];
    const int2 tile = list[blockIdx.x];
    const int a = tile.x, b = tile.y;
    const int i0 = (int)min((long long)a * bin, (long long)T), i1 = (int)min((long long)i0 + bin, (long long)T);
    const int k0 = (int)min((long long)b * bin, (long long)T), k1 = (int)min((long long)k0 + bin, (long long)T);
    const size_t cell = (size_t)a * (size_t)side + (size_t)b;
    const ig_params p = g->par[0];
    if (SHORTCUT && b > a && i1 > i0 && k1 > k0) { /* (the same for every thread of the workgroup) */
        const int la = i1 - 1;
        const int2 m = meta[la];
        const int start = max(m.x, 0);
        const int end = (int)min((long long)start + m.y, (long long)T);
        if (m.y > 0 && k0 < end && fabsf(ds[k0] - ds[la]) >= p.d_max) {
            if (threadIdx.x == 0) {
                const unsigned long long pairs = (unsigned long long)(la - max(i0, start) + 1) * (unsigned long long)(min(k1, end) - k0);
                const long long q = emap_q_far(p);
                cis_q[cell] = pairs * (unsigned long long)q;
                cis_pairs[cell] = pairs;
                ring_pairs[cell] = 0ull;
                atomicAdd(&sc[EMAP_SC_TILES_CONST], 1ull);
                raise_max(&sc[EMAP_SC_MAXQ], (unsigned long long)(q < 0 ? -q : q));
            }
            return;
        }
    }
    emap_load_tab(tab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ni = i1 - i0, nk = k1 - k0;
    unsigned long long acc = 0, n_cis = 0, n_ring = 0, mx = 0;
    if (nk >= 64 || (unsigned long long)ni * (unsigned long long)nk >= (1ull << 31)) {
        for (int i = i0 + wave; i < i1; i += EMAP_WAVES) {
            const int2 m = meta[i];
            const bool is_ring = m.y < 0;
            const int start = max(m.x, 0);
            const int end = (int)min((long long)start + (is_ring ? -(long long)m.y : (long long)m.y), (long long)k1);
            const float di = ds[i];
            for (int k = max(k0, i + 1) + lane; k < end; k += 64) {
                if (is_ring) {
                    n_ring++;
                    continue;
                }
                const long long q = ig_quantize((double)ig_rippe(fabsf(di - ds[k]), p, tab));
                acc += (unsigned long long)q;
                n_cis++;
                const unsigned long long aq = (unsigned long long)(q < 0 ? -q : q);
                mx = aq > mx ? aq : mx;
            }
        }
    } else {
        const unsigned total = (unsigned)ni * (unsigned)nk, unk = (unsigned)nk;
        for (unsigned idx = threadIdx.x; idx < total; idx += EMAP_THREADS) {
            const unsigned ii = idx / unk;
            const int i = i0 + (int)ii, k = k0 + (int)(idx - ii * unk);
            if (k <= i) continue;
            const int2 m = meta[i];
            const bool is_ring = m.y < 0;
            const long long end = (long long)max(m.x, 0) + (is_ring ? -(long long)m.y : (long long)m.y);
            if (k >= end) continue;
            if (is_ring) {
                n_ring++;
                continue;
            }
            const long long q = ig_quantize((double)ig_rippe(fabsf(ds[i] - ds[k]), p, tab));
            acc += (unsigned long long)q;
            n_cis++;
            const unsigned long long aq = (unsigned long long)(q < 0 ? -q : q);
            mx = aq > mx ? aq : mx;
        }
    }
    acc = wave_sum_u64(acc);
    n_cis = wave_sum_u64(n_cis);
    n_ring = wave_sum_u64(n_ring);
    mx = wave_max_u64(mx);
    if (lane == 0) {
        red[wave][0] = acc;
        red[wave][1] = n_cis;
        red[wave][2] = n_ring;
        red[wave][3] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EMAP_WAVES; w++) {
            acc += red[w][0];
            n_cis += red[w][1];
            n_ring += red[w][2];
            mx = red[w][3] > mx ? red[w][3] : mx;
        }
        cis_q[cell] = acc;
        cis_pairs[cell] = n_cis;
        ring_pairs[cell] = n_ring;
        atomicAdd(&sc[EMAP_SC_TILES_EVAL], 1ull);
        raise_max(&sc[EMAP_SC_MAXQ], mx);
    }
}

/* the checksum of ig_debug_expected_map_time: every word of the three images weighted by its place (wrap-around sums), one partial
 * per workgroup added to *out */
__global__ void __launch_bounds__(EMAP_THREADS) k_emap_checksum(const unsigned long long* __restrict__ img, long long n, unsigned long long* __restrict__ out)
{
    unsigned long long s = 0;
    for (long long k = (long long)blockIdx.x * EMAP_THREADS + threadIdx.x; k < n; k += (long long)gridDim.x * EMAP_THREADS)
        s += img[k] * (unsigned long long)(k + 1);
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}
