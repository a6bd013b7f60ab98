/* ig_kernels_wave.cuh -- the wave idioms: what the kernels of the reports on the current genome share below the
 * level of a kernel, each stated once.  Device helpers only.  The shuffles and the ballot need every lane: whoever calls
 * wave_runs, wave_run_sum, wave_sum_u64 or wave_max_u64 calls with whole waves (a lane with nothing to say brings no key, or 0). */
#pragma once

struct WaveRuns {
    unsigned long long heads; /* bit l: lane l is the first lane of its run (bit 0 is always set) */
    bool head;                /* this lane is */
    int run_end;              /* the first lane behind this lane's run, 64: the run reaches the end of the wave */
};

/* The runs of neighbouring lanes with an equal key: a run ends where the key changes and at the wave's last lane, whatever the next
 * wave holds.  A key that means "none" makes runs like any other: its lanes split the runs on either side. */
template <typename K>
__device__ __forceinline__ WaveRuns wave_runs(K key, int lane)
{
    WaveRuns r;
    const K left = __shfl_up(key, 1, 64);
    r.head = lane == 0 || left != key;
    r.heads = __ballot(r.head);
    const unsigned long long above = lane == 63 ? 0ull : r.heads >> (lane + 1);
    r.run_end = above ? lane + __ffsll((long long)above) : 64;
    return r;
}

/* The sum of v over this lane's run from this lane on: in the head of a run the run's total (six shuffle steps whatever the number
 * of runs).  A wave whose 64 keys all differ from their neighbours has nothing to add and skips the steps.  V: int where 64 values
 * cannot overflow one, else long long. */
template <typename V>
__device__ __forceinline__ V wave_run_sum(const WaveRuns& r, V v, int lane)
{
    if (r.heads != ~0ull) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const V o = __shfl_down(v, d, 64);
            if (lane + d < r.run_end) v += o;
        }
    }
    return v;
}

/* 64-bit reductions over the wave: every lane gets the result */
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
/* *word = max(*word, mx) for a word that only grows (the largest |quantised value| a pass saw, the host's overflow guard): whoever
 * cannot raise what is there already leaves the word alone.  One lane per wave calls. */
__device__ __forceinline__ void raise_max(unsigned long long* word, unsigned long long mx)
{
    if (mx > *(volatile unsigned long long*)word) atomicMax(word, mx);
}

/* The class scalars of a pass over the contacts, NS words of LDS per workgroup that every thread adds to once.  The head of the
 * pass: the words zeroed, every thread behind it.  The tail: every thread has added, one atomic per non-zero word. */
template <int NS>
__device__ __forceinline__ void class_zero(unsigned long long* sc)
{
    if (threadIdx.x < NS) sc[threadIdx.x] = 0ull;
    __syncthreads();
}
template <int NS>
__device__ __forceinline__ void class_flush(const unsigned long long* sc, unsigned long long* __restrict__ out_sc)
{
    __syncthreads();
    if (threadIdx.x < NS) {
        const unsigned long long v = sc[threadIdx.x];
        if (v) atomicAdd(&out_sc[threadIdx.x], v);
    }
}

/* a sharded handle takes the contacts of the rows i with i % world == rank: the ranks' integer results add up */
__device__ __forceinline__ bool contact_is_mine(int i, int rank, int world) { return world == 1 || i % world == rank; }
