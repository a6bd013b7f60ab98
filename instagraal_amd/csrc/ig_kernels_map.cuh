/* ig_kernels_map.cuh -- the contact map of the current genome (display_current_matrix, CL:2555-2605) as a binned integer image.
 *
 * The reference densifies the whole matrix (sparse_matrix.toarray()) and fancy-indexes it by the sub-fragment order of the genome;
 * at 150 k sub-fragments that is 2 10^10 entries.  Here the contacts stay where they are: every sub-fragment gets its POSITION in
 * the reference's full_order_high and from it a pixel (k_map_pixels), then one contact-parallel pass over the COO copy of the
 * contacts adds every count to the pixel pair of its two ends (k_contact_map).  64-bit integer atomics: the image is exact and
 * the same from run to run; with one sub-fragment per pixel it is the reference's matrix entry for entry (less the diagonal of
 * the input matrix: the device holds the strict upper triangle only, ig_upload_contacts).
 *
 * Nothing here writes anything a move reads. */
#pragma once

#define MAP_THREADS 256
#define MAP_TILE 32

/* One pass over the contacts (row of contact k: crow[k]; column and count: cc[k]; row-major sorted).
 *
 * COMBINE = false, the yardstick: one atomic per contact END -- image[pi][pj] and image[pj][pi] (pi == pj: twice into that pixel).
 *
 * COMBINE = true: the image is symmetric, so only image[min][max] is accumulated (k_map_mirror writes the other half and doubles
 * the diagonal), and equal destinations are combined inside the wave first: the lanes of a wave hold 64 CONSECUTIVE contacts, i.e.
 * mostly one row, and neighbouring columns fall into the same pixel -- runs of lanes with an equal key.  wave_runs finds them,
 * wave_run_sum leaves each run's total in its head (ig_kernels_wave.cuh), and only the heads issue an atomic.  V: int where 64
 * counts cannot overflow one (the host knows the largest count), else long long. */
template <bool COMBINE, typename V>
__global__ void __launch_bounds__(MAP_THREADS) k_contact_map(const int* __restrict__ crow, const int2* __restrict__ cc, long long Z,
                                                             const int* __restrict__ pix, int side, unsigned long long* __restrict__ image,
                                                             int rank, int world)
{
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * MAP_THREADS;
    const long long Zr = (Z + 63) & ~63LL; /* whole waves stay in the loop together (the shuffles need every lane) */
    for (long long k = (long long)blockIdx.x * MAP_THREADS + threadIdx.x; k < Zr; k += stride) {
        const unsigned long long none = ~0ull;
        unsigned long long key = none;
        int pi = -1, pj = -1;
        V v = 0;
        if (k < Z) {
            const int i = crow[k];
            const int2 e = cc[k];
            if (contact_is_mine(i, rank, world)) {
                pi = pix[i];
                pj = pix[e.x];
                if (pi >= 0 && pj >= 0) {
                    key = (unsigned long long)min(pi, pj) * (unsigned long long)side + (unsigned long long)max(pi, pj);
                    v = (V)e.y;
                }
            }
        }
        if (!COMBINE) {
            if (key != none) {
                const unsigned long long a = (unsigned long long)pi * (unsigned long long)side + (unsigned long long)pj;
                const unsigned long long b = (unsigned long long)pj * (unsigned long long)side + (unsigned long long)pi;
                atomicAdd(&image[a], (unsigned long long)(long long)v);
                atomicAdd(&image[b], (unsigned long long)(long long)v);
            }
            continue;
        }
        const WaveRuns runs = wave_runs(key, lane);
        v = wave_run_sum<V>(runs, v, lane);
        if (runs.head && key != none && v != 0) atomicAdd(&image[key], (unsigned long long)(long long)v);
    }
}

/* behind k_contact_map<true>: image[y][x] = image[x][y] for x < y, the diagonal doubled (a contact inside one pixel counts for both
 * of its ends).  One workgroup per 32 x 32 tile on or below the diagonal, through LDS so that both sides are row accesses. */
__global__ void __launch_bounds__(MAP_TILE * 8) k_map_mirror(unsigned long long* __restrict__ image, int side)
{
    const int tx = blockIdx.x, ty = blockIdx.y; /* the destination tile: rows ty, columns tx */
    if (tx > ty) return;
    __shared__ unsigned long long tile[MAP_TILE][MAP_TILE + 1];
    const int i = threadIdx.x;
    for (int j = threadIdx.y; j < MAP_TILE; j += 8) { /* source: rows of tile tx, columns of tile ty */
        const int sy = tx * MAP_TILE + j, sx = ty * MAP_TILE + i;
        tile[j][i] = (sy < side && sx < side) ? image[(size_t)sy * side + sx] : 0ull;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < MAP_TILE; j += 8) {
        const int y = ty * MAP_TILE + j, x = tx * MAP_TILE + i;
        if (y >= side || x >= side) continue;
        if (x < y) image[(size_t)y * side + x] = tile[i][j];
        else if (x == y) image[(size_t)y * side + x] = 2ull * tile[i][j];
    }
}
