/* ig_kernels_genome.cuh -- the genome view: the tables every report on the current genome starts from (GenomeBuf, ig_common.cuh; the
 * host side: ig_host_genome.inc).  Per sub-fragment its pixel (with one position per pixel: its position in the genome order) and
 * a 16-byte record; per position of the order the sub-fragment there, its dist and its contig.  The kernels keep the names of the
 * reports they were written for: the contact map (k_map_pixels) and the distance law (k_law_records, k_law_sorted,
 * DESIGN.md 4.11).
 *
 * Nothing here writes anything a move reads. */
#pragma once

/* position r of sub-fragment s = first position of its contig (map_base of its bin, -1: the contig is not placed) + its rank inside
 * the contig, which is Tables.cp[s].y (k_fill_tables folds the orientation in); pixel = r / bin.  order (may be null): order[r] = s. */
__global__ void k_map_pixels(const SubTab* __restrict__ sub, Tables t, const int* __restrict__ map_base, int M, int T, int bin,
                             int* __restrict__ pix, int* __restrict__ order, int* __restrict__ err)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= M) return;
    const int base = map_base[sub[s].parent];
    int p = -1;
    if (base >= 0) {
        const int r = base + t.cp[s].y;
        if ((unsigned)r < (unsigned)T) {
            if (order) order[r] = s;
            p = r / bin;
        } else
            atomicOr(err, 1); /* the tables and the state disagree: reported by the host, nothing is written out of bounds */
    }
    pix[s] = p;
}

/* one 16-byte record per sub-fragment, one gather per contact endpoint: (dist, s_tot, contig, position in the genome order or -1:
 * the contig is not placed -- the pixel table with one position per pixel) */
__global__ void k_law_records(Tables t, const int* __restrict__ pix, int M, int4* __restrict__ rec)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= M) return;
    rec[s] = make_int4(__float_as_int(t.dist[s]), __float_as_int(t.stot[s]), t.cp[s].x, pix[s]);
}

/* what the records a, b of a contact's two ends say of it, the first that fits: an end that is not placed; two contigs; one contig
 * that is a ring (s_tot != 0: a pair on it has two separations); one linear contig, the only class with a separation and with
 * positions pa <= pb.  Every pass over the contacts that reads the records keeps its own counters per class. */
enum GenomePair { PAIR_UNPLACED, PAIR_TRANS, PAIR_RING, PAIR_CIS };
__device__ __forceinline__ GenomePair genome_pair_class(const int4& a, const int4& b)
{
    if (a.w < 0 || b.w < 0) return PAIR_UNPLACED;
    if (a.z != b.z) return PAIR_TRANS;
    if (__int_as_float(a.y) != 0.0f) return PAIR_RING;
    return PAIR_CIS;
}

/* the same by POSITION r of the genome order (order[r] = sub-fragment): ds[r] = its dist, meta[r] = (first position of its contig,
 * sub-fragments of its contig; negated: a ring) */
__global__ void k_law_sorted(Tables t, const int* __restrict__ order, int M, int T, float* __restrict__ ds, int2* __restrict__ meta)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= T) return;
    const int s = order[r];
    if ((unsigned)s >= (unsigned)M) { /* (a position nobody wrote: an inconsistent state -- a contig of one, nothing read out of bounds) */
        ds[r] = 0.0f;
        meta[r] = make_int2(r, 1);
        return;
    }
    const int len = t.len[s];
    ds[r] = t.dist[s];
    meta[r] = make_int2(r - t.cp[s].y, t.stot[s] != 0.0f ? -len : len);
}
