/* ig_kernels_text.cuh -- 4DN pairs text on the device: the lines of a chunk of bytes, their fields, the two decimal
 * positions, the strand bits and the contig names.  The rule is stated once, in instagraal_amd/pairs_text.py; the passes here reproduce
 * its arrays byte for byte.
 *
 * A chunk is at most 2^30 bytes, so every offset inside it is 32-bit.  The device buffer is allocated to a multiple of 16 bytes plus 16
 * (a thread of k_text_mark loads its own 16 bytes and the 16 behind them); the bytes at index >= n_bytes are whatever the buffer held
 * and are masked BY INDEX wherever they are loaded: a pad byte never makes or alters a line.
 *
 * Here: k_text_mark (16 bytes per thread: the newline bits of the run, the per-block newline counts for the shared 64-bit scan, the
 * '\r' / >= 0x80 flag and the least offset of a line that starts with "#columns:"), k_text_lines (line_start from the block base and
 * the rank inside the block), k_text_parse (one line per thread, 256 consecutive lines per workgroup: staged once through LDS where
 * their bytes fit TEXT_LDS_SPAN, read from global memory where they do not -- one line walker, two address spaces), k_text_compact
 * (the DATA lines and the indices of the DEFERRED ones in input order) and k_text_convert (the DATA pairs as the pre store or the
 * pairs session takes them).
 *
 * Nothing here reads or writes anything a move reads or writes. */
#pragma once

#define TEXT_THREADS 256
#define TEXT_RUN 16                              /* bytes a thread of k_text_mark owns: one 16-byte load */
#define TEXT_BLOCK_BYTES (TEXT_THREADS * TEXT_RUN)
#define TEXT_LINES 256                           /* lines a workgroup of k_text_parse owns, one per thread */
/* bytes of 256 consecutive lines up to which they are staged through LDS: 128 bytes a line, above the 60 .. 120 of a pairs line with a
 * readID of ordinary length; 32 KiB (+ 16 for the aligned start) leave four workgroups to a CU's 160 KiB */
#define TEXT_LDS_SPAN 32768
#define TEXT_MAX_BYTES (1ll << 30)
#define TEXT_MAX_DIGITS 18                       /* 10^18 < 2^63: no overflow check */
#define TEXT_DATA 0
#define TEXT_COMMENT 1
#define TEXT_MALFORMED 2
#define TEXT_DEFERRED 3
/* TextBuf.sc, in 32-bit words */
#define TEXT_SC_TO_HOST 0
#define TEXT_SC_COLS_OFF 1                       /* least offset of a line that starts with "#columns:", 0xffffffff: none */
#define TEXT_SC_COLS_LINE 2                      /* its index */
#define TEXT_SC_COUNT 3                          /* + status: the lines of every status in front of the #columns: line */
#define TEXT_SC_WORDS 8
#define TEXT_FNV_BASIS 1469598103934665603ull
#define TEXT_FNV_PRIME 1099511628211ull
#define TEXT_FEED_PRE 0
#define TEXT_FEED_PAIRS 1

/* the six column indices of read_pairs and what follows from them: wave-uniform, passed by value */
struct TextCols {
    int c[6];
    int need;  /* max(c[0..3]) + 1: the fields a line must have */
    int last;  /* max(c[0..5]): no field behind it is looked at */
};

/* the vocabulary: the names' bytes one behind the other, an open-addressing table of name indices (-1: free) with a power-of-two number
 * of slots at load <= 0.5, probed linearly from the 64-bit FNV-1a hash of the field */
struct TextNames {
    const unsigned char* bytes;
    const long long* off;  /* [n + 1] */
    const int* id;         /* [n] */
    const int* table;      /* [mask + 1] */
    unsigned mask;
};

/* the per-line results in front of the compaction */
struct TextRaw {
    int *c1, *c2;
    long long *p1, *p2;
    unsigned char* strands;
};

__global__ void __launch_bounds__(TEXT_THREADS) k_text_mark(const unsigned char* __restrict__ bytes, unsigned n_bytes, unsigned short* __restrict__ nl_bits,
                                                            unsigned long long* __restrict__ blk_count, unsigned* __restrict__ sc)
{
    __shared__ unsigned s_count;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const unsigned run = blockIdx.x * TEXT_THREADS + threadIdx.x;
    const unsigned at = run * TEXT_RUN;
    unsigned nl = 0u;
    if (at < n_bytes) {
        const uint4 a = ((const uint4*)bytes)[run], b = ((const uint4*)bytes)[run + 1]; /* (both inside the allocation: a multiple of 16, plus 16) */
        const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const unsigned live = min(n_bytes - at, 16u);
        unsigned bad = 0u, hash_bits = 0u;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const unsigned ch = (w[i >> 2] >> ((i & 3) * 8)) & 0xffu;
            const unsigned in = (unsigned)i < live ? 1u : 0u; /* masked by index, not by a pad value */
            nl |= (in & (ch == '\n' ? 1u : 0u)) << i;
            bad |= in & ((ch == '\r' || ch >= 0x80u) ? 1u : 0u);
            hash_bits |= (in & (ch == '#' ? 1u : 0u)) << i;
        }
        if (bad) atomicOr(&sc[TEXT_SC_TO_HOST], 1u);
        if (hash_bits) { /* rare: a '#' at the start of a line with "columns:" behind it, all of it inside the chunk */
            const unsigned prev_nl = at == 0u ? 1u : (bytes[at - 1] == '\n' ? 1u : 0u);
            unsigned starts = hash_bits & ((nl << 1) | prev_nl);
            while (starts) {
                const int i = __ffs((int)starts) - 1;
                starts &= starts - 1u;
                if (at + (unsigned)i + 9u > n_bytes) continue;
                const char* word = "columns:";
                bool same = true;
                for (int k = 0; k < 8; k++) {
                    const int q = i + 1 + k; /* < 25: inside the two loads */
                    same = same && ((w[q >> 2] >> ((q & 3) * 8)) & 0xffu) == (unsigned)word[k];
                }
                if (same) atomicMin(&sc[TEXT_SC_COLS_OFF], at + (unsigned)i);
            }
        }
        nl_bits[run] = (unsigned short)nl;
    }
    if (nl) atomicAdd(&s_count, (unsigned)__popc(nl));
    __syncthreads();
    if (threadIdx.x == 0) blk_count[blockIdx.x] = (unsigned long long)s_count;
}

/* the inclusive prefix sum of v over the workgroup's threads, in thread order; s_wave: TEXT_THREADS / 64 words */
__device__ __forceinline__ unsigned text_block_scan(unsigned v, unsigned* s_wave)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    for (int k = 0; k < wave; k++) incl += s_wave[k];
    __syncthreads();
    return incl;
}

/* line_start[r + 1] = the byte behind the r-th newline; line_start[0] = 0 and line_start[n_lines] = n_bytes (a last line without a
 * newline).  blk_incl: the inclusive prefix sums of blk_count */
__global__ void __launch_bounds__(TEXT_THREADS) k_text_lines(const unsigned short* __restrict__ nl_bits, unsigned n_bytes, const unsigned long long* __restrict__ blk_incl,
                                                             int* __restrict__ line_start, unsigned n_lines)
{
    __shared__ unsigned s_wave[TEXT_THREADS / 64];
    const unsigned run = blockIdx.x * TEXT_THREADS + threadIdx.x;
    const unsigned at = run * TEXT_RUN;
    unsigned nl = at < n_bytes ? (unsigned)nl_bits[run] : 0u;
    const unsigned incl = text_block_scan((unsigned)__popc(nl), s_wave);
    unsigned rank = (unsigned)(blockIdx.x ? blk_incl[blockIdx.x - 1] : 0ull) + incl - (unsigned)__popc(nl);
    while (nl) {
        const int i = __ffs((int)nl) - 1;
        nl &= nl - 1u;
        if (rank + 1u <= n_lines) line_start[rank + 1u] = (int)(at + (unsigned)i + 1u);
        rank++;
    }
    if (run == 0u) {
        line_start[0] = 0;
        line_start[n_lines] = (int)n_bytes;
    }
}

/* [a, b) of the line's bytes -> its value where it is exactly [+-]?[0-9]{1,18}; p[i - bias] is byte i of the chunk */
__device__ __forceinline__ bool text_int(const unsigned char* p, unsigned bias, unsigned a, unsigned b, long long* out)
{
    bool minus = false;
    if (a < b && (p[a - bias] == '+' || p[a - bias] == '-')) minus = p[a - bias] == '-', a++;
    if (a >= b || b - a > TEXT_MAX_DIGITS) return false;
    long long v = 0;
    for (unsigned i = a; i < b; i++) {
        const unsigned d = (unsigned)p[i - bias] - '0';
        if (d > 9u) return false;
        v = v * 10 + (long long)d;
    }
    *out = minus ? -v : v;
    return true;
}

/* the id of the name that is exactly the bytes [a, b), -1: none */
__device__ __forceinline__ int text_name(const unsigned char* p, unsigned bias, unsigned a, unsigned b, const TextNames& names)
{
    unsigned long long h = TEXT_FNV_BASIS;
    for (unsigned i = a; i < b; i++) h = (h ^ (unsigned long long)p[i - bias]) * TEXT_FNV_PRIME;
    for (unsigned slot = (unsigned)h & names.mask, probes = 0; probes <= names.mask; slot = (slot + 1u) & names.mask, probes++) {
        const int k = names.table[slot];
        if (k < 0) return -1;
        const long long o = names.off[k];
        if (names.off[k + 1] - o != (long long)(b - a)) continue;
        bool same = true;
        for (unsigned i = a; i < b && same; i++) same = names.bytes[o + (i - a)] == p[i - bias];
        if (same) return names.id[k]; /* (a hit is confirmed by the bytes) */
    }
    return -1;
}

/* One line: the bytes [a, e) without its newline -> its status; the fields of a DATA line */
__device__ __forceinline__ int text_line(const unsigned char* p, unsigned bias, unsigned a, unsigned e, const TextCols& cols, const TextNames& names, int* c1, long long* p1,
                                         int* c2, long long* p2, unsigned* strand)
{
    if (a < e && p[a - bias] == '#') return TEXT_COMMENT;
    unsigned fs[6], fe[6];
#pragma unroll
    for (int k = 0; k < 6; k++) fs[k] = fe[k] = a;
    int f = 0;
    unsigned start = a;
    for (unsigned i = a; i <= e; i++) { /* (an empty line is one empty field) */
        if (i < e && p[i - bias] != '\t') continue;
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (f == cols.c[k]) fs[k] = start, fe[k] = i;
        f++;
        start = i + 1u;
        if (f > cols.last) break; /* the fields behind the last column decide nothing */
    }
    if (f < cols.need) return TEXT_MALFORMED;
    if (!text_int(p, bias, fs[1], fe[1], p1) || !text_int(p, bias, fs[3], fe[3], p2)) return TEXT_DEFERRED;
    *strand = ((cols.c[4] < f && fe[4] - fs[4] == 1u && p[fs[4] - bias] == '-') ? 1u : 0u) | ((cols.c[5] < f && fe[5] - fs[5] == 1u && p[fs[5] - bias] == '-') ? 2u : 0u);
    *c1 = text_name(p, bias, fs[0], fe[0], names);
    *c2 = text_name(p, bias, fs[2], fe[2], names);
    return TEXT_DATA;
}

/* Workgroup b owns the lines 256 b .. 256 b + 255, one per thread.  Where their bytes fit TEXT_LDS_SPAN
 * they are staged once with 16-byte loads from the aligned start, and the lines are walked in LDS; else they are walked in global
 * memory.  A line at or behind the first "#columns:" line is left COMMENT and counted nowhere.  blk_count: [2][n_blocks], the DATA and
 * the DEFERRED lines of every workgroup. */
__global__ void __launch_bounds__(TEXT_THREADS) k_text_parse(const unsigned char* __restrict__ bytes, unsigned n_bytes, const int* __restrict__ line_start, unsigned n_lines,
                                                             TextCols cols, TextNames names, unsigned char* __restrict__ status, TextRaw raw,
                                                             unsigned long long* __restrict__ blk_count, unsigned n_blocks, unsigned* __restrict__ sc)
{
    __shared__ uint4 s_stage[TEXT_LDS_SPAN / 16 + 1];
    __shared__ unsigned s_count[4];
    const unsigned first = blockIdx.x * TEXT_LINES, line = first + threadIdx.x;
    const unsigned lo = (unsigned)line_start[first], hi = (unsigned)line_start[min(first + TEXT_LINES, n_lines)];
    const bool staged = hi - lo <= (unsigned)TEXT_LDS_SPAN;
    const unsigned lo16 = lo & ~15u;
    if (threadIdx.x < 4) s_count[threadIdx.x] = 0u;
    if (staged)
        for (unsigned q = threadIdx.x; lo16 + 16u * q < hi; q += TEXT_THREADS) s_stage[q] = ((const uint4*)bytes)[(lo16 >> 4) + q]; /* (hi <= n_bytes: inside the allocation) */
    __syncthreads();
    int st = -1;
    if (line < n_lines) {
        const unsigned a = (unsigned)line_start[line];
        unsigned e = (unsigned)line_start[line + 1];
        const unsigned cols_off = sc[TEXT_SC_COLS_OFF];
        if (a >= cols_off) {
            st = TEXT_COMMENT;
            if (a == cols_off) sc[TEXT_SC_COLS_LINE] = line;
            status[line] = TEXT_COMMENT;
        } else {
            int c1 = -1, c2 = -1;
            long long p1 = 0, p2 = 0;
            unsigned strand = 0u;
            if (staged) {
                const unsigned char* p = (const unsigned char*)s_stage;
                if (e > a && p[e - 1u - lo16] == '\n') e--;
                st = text_line(p, lo16, a, e, cols, names, &c1, &p1, &c2, &p2, &strand);
            } else {
                if (e > a && bytes[e - 1u] == '\n') e--;
                st = text_line(bytes, 0u, a, e, cols, names, &c1, &p1, &c2, &p2, &strand);
            }
            status[line] = (unsigned char)st;
            if (st == TEXT_DATA) raw.c1[line] = c1, raw.p1[line] = p1, raw.c2[line] = c2, raw.p2[line] = p2, raw.strands[line] = (unsigned char)strand;
            atomicAdd(&s_count[st], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(&sc[TEXT_SC_COUNT + threadIdx.x], s_count[threadIdx.x]);
    if (threadIdx.x == 0) {
        blk_count[blockIdx.x] = (unsigned long long)s_count[TEXT_DATA];
        blk_count[n_blocks + blockIdx.x] = (unsigned long long)s_count[TEXT_DEFERRED];
    }
}

/* the DATA lines into the session's arrays and the indices of the DEFERRED lines, both in input order.  blk_incl: [2][n_blocks], the
 * inclusive prefix sums of k_text_parse's counts; n_data, n_deferred: what the arrays hold (nothing is written beyond them) */
__global__ void __launch_bounds__(TEXT_THREADS) k_text_compact(const unsigned char* __restrict__ status, unsigned n_lines, unsigned cols_line, TextRaw raw,
                                                               const unsigned long long* __restrict__ blk_incl, unsigned n_blocks, TextRaw out, unsigned n_data,
                                                               int* __restrict__ deferred, unsigned n_deferred)
{
    __shared__ unsigned s_wave[TEXT_THREADS / 64];
    const unsigned line = blockIdx.x * TEXT_LINES + threadIdx.x;
    const int st = line < n_lines && line < cols_line ? (int)status[line] : -1;
    const unsigned is_data = st == TEXT_DATA ? 1u : 0u, is_def = st == TEXT_DEFERRED ? 1u : 0u;
    const unsigned incl = text_block_scan(is_data | (is_def << 16), s_wave); /* (two counts of at most 256 in one word) */
    if (is_data) {
        const unsigned at = (unsigned)(blockIdx.x ? blk_incl[blockIdx.x - 1] : 0ull) + (incl & 0xffffu) - 1u;
        if (at < n_data) out.c1[at] = raw.c1[line], out.p1[at] = raw.p1[line], out.c2[at] = raw.c2[line], out.p2[at] = raw.p2[line], out.strands[at] = raw.strands[line];
    }
    if (is_def) {
        const unsigned at = (unsigned)(blockIdx.x ? blk_incl[n_blocks + blockIdx.x - 1] : 0ull) + (incl >> 16) - 1u;
        if (at < n_deferred) deferred[at] = (int)line;
    }
}

/* the DATA pairs first .. first + m - 1 as a piece of a chunk: for the pre store the positions clipped to 0 .. 2^31 - 1 (pre._clip32),
 * for the pairs session a position outside 1 .. 2^31 - 1 as 0 and a negative id as -1 (Context.pairs_lift), with the strand codes */
__global__ void __launch_bounds__(TEXT_THREADS) k_text_convert(TextRaw data, long long first, long long m, int mode, int* __restrict__ c1, int* __restrict__ p1,
                                                               int* __restrict__ c2, int* __restrict__ p2, unsigned char* __restrict__ strands)
{
    const long long stride = (long long)gridDim.x * TEXT_THREADS;
    for (long long k = (long long)blockIdx.x * TEXT_THREADS + threadIdx.x; k < m; k += stride) {
        const long long a = data.p1[first + k], b = data.p2[first + k];
        const int x = data.c1[first + k], y = data.c2[first + k];
        if (mode == TEXT_FEED_PRE) {
            c1[k] = x, c2[k] = y;
            p1[k] = (int)min(max(a, 0ll), 0x7fffffffll), p2[k] = (int)min(max(b, 0ll), 0x7fffffffll);
        } else {
            c1[k] = x < 0 ? -1 : x, c2[k] = y < 0 ? -1 : y;
            p1[k] = (a < 1 || a > 0x7fffffffll) ? 0 : (int)a, p2[k] = (b < 1 || b > 0x7fffffffll) ? 0 : (int)b;
            strands[k] = data.strands[first + k];
        }
    }
}
