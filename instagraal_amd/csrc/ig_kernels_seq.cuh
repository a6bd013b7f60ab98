/* ig_kernels_seq.cuh -- the polished FASTA of the polish step: the composition of the input records and the
 * stitching of the output file from the input bases.  The rule is stated once, in instagraal_amd/scaffold_polish.py (composition,
 * stitch_plan, stitch); the two kernels here reproduce its bytes and counts exactly.
 *
 * The input is the layout of ig_pre_begin: the records one behind the other in ONE 64-bit coordinate, a zero byte behind each; here
 * with 16 zero bytes in front as well, so that the aligned 16-byte words around any base of the sequence lie inside the allocation.
 * The output file is a second 64-bit coordinate: per output record a header (bytes of a small literal buffer), then the body, a
 * newline behind every `width` bases and behind the last line.  A body is tiled by pieces: a run of a source record, forward or as its
 * reverse complement, or a run of the literal buffer (a junction).
 *
 * k_seq_composition: 16 bytes per thread and turn, eight classes per byte (SEQ_NC), summed per thread while its record stays the same
 * (a wave walks a stretch of consecutive kilobytes), then per wave and record run; one atomic per class, wave and run.  k_seq_stitch: a thread owns 16 consecutive file bytes and makes
 * one 16-byte store; a wave walks consecutive kilobytes, so the record and the piece of the turn before are nearly always those of
 * this turn and the two binary searches are skipped.
 *
 * Plain C++, vector loads and stores, ordinary atomics.  Nothing here reads or writes anything a move reads or writes. */
#pragma once

#define SEQ_THREADS 256
#define SEQ_RUN 16     /* file bytes (sequence bytes) a thread owns per turn */
#define SEQ_NC 8       /* scaffold_polish.CLASSES: A, C, G, T, N of either case, other letters, lower case, all bases */
#define SEQ_FRONT 16   /* zero bytes in front of the sequence */
#define SEQ_PIECE_REVERSE 1
#define SEQ_PIECE_LITERAL 2
#define SEQ_COMP_MAX_TURNS (1 << 20) /* turns of a wave of k_seq_composition: 2^20 * 16 * 64 = 2^30 per class and wave at the most */

/* The per-thread work is written as host-and-device functions: the sanitizer harness (tests/sanitize/seq_harness.cpp) includes this
 * file with SEQ_HOST_MODEL defined, leaves the kernels and the wave step out, and runs these very functions over the fake device heap. */
#define SEQ_HD __host__ __device__ __forceinline__

typedef unsigned __int128 seq_u128;

struct SeqPiece {
    long long addr; /* of its first source byte: in the sequence coordinate, or in the literal buffer */
    int len, flags;
};

/* the plan of one output file: wave-uniform, passed by value */
struct SeqPlan {
    const long long* rec_off;     /* [n_out + 1] the file offset of every header, the file's size last */
    const int* hdr_len;           /* [n_out] */
    const long long* hdr_lit;     /* [n_out] where the header lies in lit */
    const long long* piece_first; /* [n_out + 1] */
    const long long* p_body;      /* [n_pieces] the offset of a piece's first base in its record's body */
    const SeqPiece* piece;        /* [n_pieces] */
    const unsigned char* lit;
    long long file_bytes;
    int n_out, width;
};

/* a byte -> what it adds to the eight classes, 8 bits each (0: no letter of ABCDGHKMNRSTVWY) */
SEQ_HD unsigned long long seq_class(unsigned b)
{
    const unsigned i = (b & 0x1fu) - 1u;
    if ((b & 0xc0u) != 0x40u || i >= 26u || !((PRE_LETTERS >> i) & 1u)) return 0ull;
    const int cls = i == 0u ? 0 : i == 2u ? 1 : i == 6u ? 2 : i == 19u ? 3 : i == 13u ? 4 : 5;
    return (1ull << (8 * cls)) | ((unsigned long long)((b >> 5) & 1u) << 48) | (1ull << 56);
}

/* Biopython's ambiguous_dna_complement over the letters of the alphabet, the case kept; every other byte is itself */
SEQ_HD unsigned seq_complement(unsigned b)
{
    const unsigned i = (b & 0x1fu) - 1u;
    if ((b & 0xc0u) != 0x40u || i >= 26u || !((PRE_LETTERS >> i) & 1u)) return b;
    return (unsigned)(unsigned char)"TVGHEFCDIJMLKNOPQYSAUBWXRZ"[i] | (b & 0x20u);
}

SEQ_HD unsigned long long seq_class16(seq_u128 v)
{
    unsigned long long s = 0ull;
#pragma unroll
    for (int i = 0; i < 16; i++) s += seq_class((unsigned)(v >> (8 * i)) & 0xffu);
    return s; /* (16 at the most per class: 8 bits hold it) */
}

/* A thread's counts for the record `key` (-1: none yet): four words of two 32-bit sums.  A thread whose record changes adds what it
 * has by itself; what it holds at the end goes through the wave (seq_counts_flush). */
struct SeqCounts {
    long long key;
    unsigned long long w[4];
};

SEQ_HD void seq_count_word(unsigned long long* p, unsigned long long v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v; /* (the host model: one thread) */
#endif
}

SEQ_HD void seq_counts_own(const SeqCounts& s, unsigned long long* __restrict__ counts)
{
    if (s.key < 0) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long lo = s.w[k] & 0xffffffffull, hi = s.w[k] >> 32;
        if (lo) seq_count_word(&counts[s.key * SEQ_NC + 2 * k], lo);
        if (hi) seq_count_word(&counts[s.key * SEQ_NC + 2 * k + 1], hi);
    }
}

SEQ_HD void seq_counts_add(SeqCounts& s, long long key, unsigned long long packed, unsigned long long* __restrict__ counts)
{
    if (!packed) return;
    if (key != s.key) {
        seq_counts_own(s, counts);
        s.key = key;
        s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0ull;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) s.w[k] += ((packed >> (16 * k)) & 0xffull) | (((packed >> (16 * k + 8)) & 0xffull) << 32);
}

#ifndef SEQ_HOST_MODEL
/* every lane of the wave calls: the runs of neighbouring lanes with one record add up, the head of a run adds the run's sums */
__device__ __forceinline__ void seq_counts_flush(SeqCounts& s, unsigned long long* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const WaveRuns runs = wave_runs(s.key, lane);
#pragma unroll
    for (int k = 0; k < 4; k++) s.w[k] = wave_run_sum(runs, s.w[k], lane); /* (a lane holds less than 2^25 per class, a wave less than 2^31) */
    if (runs.head) seq_counts_own(s, counts);
}
#endif

/* the largest i of [lo, hi) with a[i] <= x, where a ascends and a[lo] <= x */
SEQ_HD long long seq_search(const long long* __restrict__ a, long long lo, long long hi, long long x)
{
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* the 16 bytes at a .. a + 15 of the sequence coordinate (-16 < a, a + 15 inside the padding behind): two aligned words and a shift */
SEQ_HD seq_u128 seq_load16(const unsigned char* __restrict__ seq, long long a)
{
    const uint4* w = (const uint4*)seq + (a >> 4); /* (an arithmetic shift: the word in front of the sequence for -16 < a < 0) */
    const uint4 x = w[0], y = w[1];
    const seq_u128 lo = ((seq_u128)(((unsigned long long)x.w << 32) | x.z) << 64) | (((unsigned long long)x.y << 32) | x.x);
    const seq_u128 hi = ((seq_u128)(((unsigned long long)y.w << 32) | y.z) << 64) | (((unsigned long long)y.y << 32) | y.x);
    const int sh = (int)(a & 15) * 8;
    return sh ? (lo >> sh) | (hi << (128 - sh)) : lo;
}

/* run t of the sequence: the classes of its 16 bytes to the records they lie in */
SEQ_HD void seq_composition_run(const unsigned char* __restrict__ seq, long long t, const long long* __restrict__ off, int R, SeqCounts& acc,
                                unsigned long long* __restrict__ counts)
{
    const uint4 x = ((const uint4*)seq)[t];
    const seq_u128 v = ((seq_u128)(((unsigned long long)x.w << 32) | x.z) << 64) | (((unsigned long long)x.y << 32) | x.x);
    const long long p0 = t * SEQ_RUN;
    long long r = seq_search(off, 0, R, p0);
    if (r + 1 >= R || off[r + 1] >= p0 + SEQ_RUN) { /* one record (and perhaps its separator, which is no letter) */
        seq_counts_add(acc, r, seq_class16(v), counts);
    } else {
        for (int i = 0; i < SEQ_RUN; i++) {
            while (r + 1 < R && p0 + i >= off[r + 1]) r++;
            seq_counts_add(acc, r, seq_class((unsigned)(v >> (8 * i)) & 0xffu), counts);
        }
    }
}

/* the record and the piece a thread is in, kept in registers from turn to turn (j, p: -1 for none yet) */
struct SeqState {
    long long j, rec0, rec_end, pf, pe; /* the record, its first file byte and the first behind it, its pieces */
    long long p, pb;                    /* the piece and the body offset of its first base */
    SeqPiece pc;
    int h;                              /* the header's length */
};

SEQ_HD void seq_enter_record(const SeqPlan& pl, SeqState& st, long long j)
{
    st.j = j, st.rec0 = pl.rec_off[j], st.rec_end = pl.rec_off[j + 1], st.h = pl.hdr_len[j];
    st.pf = pl.piece_first[j], st.pe = pl.piece_first[j + 1], st.p = -1;
}

SEQ_HD void seq_enter_piece(const SeqPlan& pl, SeqState& st, long long p)
{
    st.p = p, st.pb = pl.p_body[p], st.pc = pl.piece[p];
}

/* The 16 file bytes from f0 on (zero behind the file's end).  st: the record and the piece of the turn before.  COUNT: the
 * classes of the body bases go to acc / out_counts.
 *
 * The fast path: the 16 bytes lie in one body, short of its last byte, with at most one newline among them (width >= 15), and their
 * 15 or 16 bases in one piece of the sequence: one unaligned 16-byte read, reversed and complemented through the table (in LDS) for a
 * reversed piece, the newline shifted in.  Everything else (headers, junctions, the ends of pieces and bodies, narrow lines) goes byte
 * by byte. */
template <bool COUNT>
SEQ_HD seq_u128 seq_stitch_run(const unsigned char* __restrict__ seq, const SeqPlan& pl, const unsigned char* comp, long long f0, SeqState& st, SeqCounts& acc,
                               unsigned long long* __restrict__ out_counts)
{
    const long long W1 = (long long)pl.width + 1;
    seq_u128 o = 0;
    if (f0 < pl.file_bytes) {
        if (st.j < 0 || f0 < st.rec0 || f0 >= st.rec_end) seq_enter_record(pl, st, seq_search(pl.rec_off, 0, pl.n_out, f0));
        const long long q0 = f0 - st.rec0 - st.h;
        const long long body_bytes = st.rec_end - st.rec0 - st.h;
        bool fast = q0 >= 0 && pl.width >= 15 && q0 + 15 < body_bytes - 1;
        if (fast) {
            const long long k = (q0 >> 32) ? q0 / W1 : (long long)((unsigned)q0 / (unsigned)W1);
            const int nl = (int)(pl.width - (q0 - k * W1)); /* where the newline stands among the 16 bytes, if below 16 */
            const int nb = nl <= 15 ? 15 : 16;
            const long long b0 = q0 - k;
            if (st.p < 0 || b0 < st.pb || b0 >= st.pb + st.pc.len) seq_enter_piece(pl, st, seq_search(pl.p_body, st.pf, st.pe, b0));
            const SeqPiece pc = st.pc;
            const long long koff = b0 - st.pb;
            fast = !(pc.flags & SEQ_PIECE_LITERAL) && koff + nb <= pc.len;
            if (fast) {
                seq_u128 s;
                if (!(pc.flags & SEQ_PIECE_REVERSE)) {
                    s = seq_load16(seq, pc.addr + koff);
                } else { /* the 16 bytes that END at the piece's base koff from its end, backwards */
                    const seq_u128 v = seq_load16(seq, pc.addr + pc.len - koff - 16);
                    s = 0;
#pragma unroll
                    for (int i = 0; i < 16; i++) s |= (seq_u128)comp[(unsigned)(v >> (8 * (15 - i))) & 0xffu] << (8 * i);
                }
                if (nb == 15) s &= ~(seq_u128)0 >> 8;
                if (COUNT) seq_counts_add(acc, st.j, seq_class16(s), out_counts);
                if (nl <= 15) {
                    const seq_u128 low = nl ? s & (((seq_u128)1 << (8 * nl)) - 1) : 0;
                    const seq_u128 high = nl < 15 ? (s >> (8 * nl)) << (8 * (nl + 1)) : 0;
                    s = low | ((seq_u128)10 << (8 * nl)) | high;
                }
                o = s;
            }
        }
        if (!fast) {
            for (int i = 0; i < SEQ_RUN; i++) {
                const long long f = f0 + i;
                if (f >= pl.file_bytes) break;
                if (f >= st.rec_end) {
                    long long j = st.j + 1;
                    while (f >= pl.rec_off[j + 1]) j++;
                    seq_enter_record(pl, st, j);
                }
                const long long hh = f - st.rec0;
                unsigned byte;
                if (hh < st.h) {
                    byte = pl.lit[pl.hdr_lit[st.j] + hh];
                } else {
                    const long long q = hh - st.h, k = q / W1;
                    if (q - k * W1 == pl.width || q == st.rec_end - st.rec0 - st.h - 1) {
                        byte = 10u;
                    } else {
                        const long long b = q - k;
                        if (st.p < 0 || b < st.pb) seq_enter_piece(pl, st, seq_search(pl.p_body, st.pf, st.pe, b));
                        while (b >= st.pb + st.pc.len) seq_enter_piece(pl, st, st.p + 1);
                        const SeqPiece pc = st.pc;
                        const long long koff = b - st.pb;
                        if (pc.flags & SEQ_PIECE_LITERAL) byte = pl.lit[pc.addr + koff];
                        else if (pc.flags & SEQ_PIECE_REVERSE) byte = comp[seq[pc.addr + pc.len - 1 - koff]];
                        else byte = seq[pc.addr + koff];
                        if (COUNT) seq_counts_add(acc, st.j, seq_class(byte), out_counts);
                    }
                }
                o |= (seq_u128)byte << (8 * i);
            }
        }
    }
    return o;
}

#ifndef SEQ_HOST_MODEL
/* counts[R][SEQ_NC] += the classes of the bytes of every record.  A wave takes runs_per_wave (at most SEQ_COMP_MAX_TURNS: the 32-bit
 * sums) consecutive turns of 64 runs: only the waves whose stretch holds a record's end ever change their record in mid-walk. */
__global__ void __launch_bounds__(SEQ_THREADS) k_seq_composition(const unsigned char* __restrict__ seq, long long n_runs, const long long* __restrict__ off, int R,
                                                                 long long runs_per_wave, unsigned long long* __restrict__ counts)
{
    SeqCounts acc = {-1ll, {0ull, 0ull, 0ull, 0ull}};
    const long long wave = (long long)blockIdx.x * (SEQ_THREADS / 64) + (threadIdx.x >> 6);
    const long long first = wave * runs_per_wave * 64 + (threadIdx.x & 63);
    for (long long turn = 0; turn < runs_per_wave; turn++) {
        const long long t = first + turn * 64;
        if (t >= n_runs) break;
        seq_composition_run(seq, t, off, R, acc, counts);
    }
    seq_counts_flush(acc, counts);
}

/* The file bytes first_byte .. first_byte + 16 n_runs - 1 (first_byte a multiple of 16) into out.  A wave takes runs_per_wave
 * consecutive turns of 64 runs, so that the record and the piece of a turn are nearly always those of the turn before. */
template <bool COUNT>
__global__ void __launch_bounds__(SEQ_THREADS) k_seq_stitch(const unsigned char* __restrict__ seq, SeqPlan pl, long long first_byte, long long n_runs, int runs_per_wave,
                                                            uint4* __restrict__ out, unsigned long long* __restrict__ out_counts)
{
    __shared__ unsigned char comp[256];
    comp[threadIdx.x] = (unsigned char)seq_complement(threadIdx.x); /* (SEQ_THREADS == 256) */
    __syncthreads();
    SeqCounts acc = {-1ll, {0ull, 0ull, 0ull, 0ull}};
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (SEQ_THREADS / 64) + (threadIdx.x >> 6);
    SeqState st;
    st.j = st.p = -1;
    for (int turn = 0; turn < runs_per_wave; turn++) {
        const long long t = (wave * runs_per_wave + turn) * 64 + lane;
        if (t >= n_runs) break;
        const seq_u128 o = seq_stitch_run<COUNT>(seq, pl, comp, first_byte + t * SEQ_RUN, st, acc, out_counts);
        out[t] = make_uint4((unsigned)o, (unsigned)(o >> 32), (unsigned)(o >> 64), (unsigned)(o >> 96));
    }
    if (COUNT) seq_counts_flush(acc, out_counts); /* (behind the loop: every lane of the wave is here) */
}
#endif
