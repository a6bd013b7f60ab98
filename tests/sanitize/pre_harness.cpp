// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the input folder from a FASTA and read pairs
// (csrc/ig_host_pre.inc: the session, the upload in pieces, the digest's bitmaps and scans, the fragment table, the store and its growth,
// the staging of a chunk, the pixels through the row builder) with the sort and reduction it shares with the reports
// (csrc/ig_host_rows.inc): a stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy,
// fill and model write is checked against the real allocation sizes).  The models below do what the seven kernels do, load for load and
// word for word -- a run's two 16-byte loads, the OR into the next bitmap word, the prefix counts read for G+C -- so the padding of the
// sequence, the sizes of the bitmaps, of the fragment table, of the store behind every growth and of the staging arrays are all
// exercised, and the digest that comes out is compared with a per-base brute force.  A second genome lies across the coordinate 2^32
// (beyond_4gib: 4 GiB of host memory and as much "device" memory; it takes about a minute).  Built and run by tests/test_pre_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_rows.cuh, ig_kernels_pre.cuh: device code, not included here)
struct Item {
    long long off;
    int len, pad;
};
struct Long {
    long long off, scratch, len;
};
struct Sites {
    int n;
    int len[4], cut[4];
    unsigned char mask[4][16];
};

static bool g_no_heads = false;
static bool g_lose_a_pair = false; // the assign pass counts a pair less than it was given: a device error the host must catch
static bool g_lose_a_cut = false;  // the marks are not set: fewer cuts than two per record
static size_t g_free_bytes = (size_t)1 << 34;
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static unsigned code_of(unsigned char b)
{
    const char* letters = "ABCDGHKMNRSTVWY";
    const int up = b >= 'a' && b <= 'z' ? b - 32 : b;
    if (!up || !std::strchr(letters, up)) return 0;
    return 16u | (up == 'A' ? 1u : 0u) | (up == 'C' ? 2u : 0u) | (up == 'G' ? 4u : 0u) | (up == 'T' ? 8u : 0u);
}
static void model_sites(void** a, dim3, dim3)
{
    const unsigned char* seq = *(const unsigned char**)a[0];
    const long long n_runs = *(long long*)a[1];
    const Sites st = *(Sites*)a[2];
    u64* cutbits = *(u64**)a[3];
    unsigned short* gcbits = *(unsigned short**)a[4];
    bool a_starts_no_site = true; // no site begins with a letter that accepts A: a run of sixteen A holds no start and no G or C
    for (int e = 0; e < st.n; e++) a_starts_no_site = a_starts_no_site && !(st.mask[e][0] & 17u);
    for (long long t = 0; t < n_runs; t++) {
        unsigned char b[32];
        if (a_starts_no_site) { // (the genome beyond 2^32 bytes is A but for a few hundred bases: its runs of A are skipped, not modelled)
            uint64_t q[2];
            __builtin_memcpy(q, seq + 16 * t, 16);
            if (q[0] == 0x4141414141414141ull && q[1] == 0x4141414141414141ull) continue;
        }
        std::memcpy(b, seq + 16 * t, 16);      // the run's own load ...
        std::memcpy(b + 16, seq + 16 * (t + 1), 16); // ... and the halo's
        unsigned cuts = 0, gc = 0;
        for (int s = 0; s < 16; s++) {
            if (code_of(b[s]) & 6u) gc |= 1u << s;
            for (int e = 0; e < st.n; e++) {
                bool ok = true;
                for (int j = 0; j < st.len[e]; j++) ok = ok && (code_of(b[s + j]) & st.mask[e][j]);
                if (ok) cuts |= 1u << (s + st.cut[e]);
            }
        }
        if (cuts) {
            const int sh = (int)(t & 3) * 16;
            const u64 lo = (u64)cuts << sh, hi = sh > 32 ? (u64)(cuts >> (64 - sh)) : 0;
            if (lo) cutbits[t >> 2] |= lo;
            if (hi) cutbits[(t >> 2) + 1] |= hi;
        }
        gcbits[t] = (unsigned short)gc;
    }
}
static void model_marks(void** a, dim3, dim3)
{
    const long long* off = *(const long long**)a[0];
    const int* len = *(const int**)a[1];
    const int R = *(int*)a[2];
    u64* cutbits = *(u64**)a[3];
    if (g_lose_a_cut) return;
    for (int r = 0; r < R; r++) {
        const long long x = off[r], y = x + len[r];
        cutbits[x >> 6] |= 1ull << (x & 63);
        cutbits[y >> 6] |= 1ull << (y & 63);
    }
}
static void model_popc(void** a, dim3, dim3)
{
    const u64 *cutbits = *(const u64**)a[0], *gcbits = *(const u64**)a[1];
    const long long W = *(long long*)a[2];
    u64* cnt = *(u64**)a[3];
    for (long long w = 0; w < W; w++) cnt[w] = (u64)__builtin_popcountll(cutbits[w]), cnt[W + w] = (u64)__builtin_popcountll(gcbits[w]);
}
static void model_cuts(void** a, dim3, dim3)
{
    const u64 *cutbits = *(const u64**)a[0], *incl = *(const u64**)a[1];
    const long long W = *(long long*)a[2];
    long long* cuts = *(long long**)a[3];
    const long long n_cuts = *(long long*)a[4];
    for (long long w = 0; w < W; w++) {
        if (!cutbits[w]) continue;
        long long rank = (long long)incl[w] - __builtin_popcountll(cutbits[w]);
        for (int b = 0; b < 64; b++)
            if ((cutbits[w] >> b) & 1) {
                if (rank >= 0 && rank < n_cuts) cuts[rank] = w * 64 + b;
                rank++;
            }
    }
}
static long long gc_before(const u64* gcbits, const u64* gcincl, long long x)
{
    const long long w = x >> 6;
    return (w ? (long long)gcincl[w - 1] : 0) + __builtin_popcountll(gcbits[w] & ((1ull << (x & 63)) - 1ull));
}
static void model_frags(void** a, dim3, dim3)
{
    const long long* cuts = *(const long long**)a[0];
    const long long n_cuts = *(long long*)a[1];
    const long long* off = *(const long long**)a[2];
    const int* len = *(const int**)a[3];
    const int R = *(int*)a[4];
    const u64 *gcbits = *(const u64**)a[5], *gcincl = *(const u64**)a[6];
    const long long n_frags = *(long long*)a[7];
    long long* rec_first = *(long long**)a[8];
    int *frag_rec = *(int**)a[9], *start = *(int**)a[10], *end = *(int**)a[11], *gc = *(int**)a[12];
    for (long long g = 0; g < n_cuts; g++) {
        const long long x = cuts[g];
        int r = -1;
        for (int k = 0; k < R; k++)
            if (off[k] <= x) r = k;
        if (r < 0 || x == off[r] + len[r]) continue;
        const long long f = g - r;
        if (f < 0 || f >= n_frags || g + 1 >= n_cuts) continue;
        const long long y = cuts[g + 1];
        if (x == off[r]) rec_first[r] = f;
        frag_rec[f] = r, start[f] = (int)(x - off[r]), end[f] = (int)(y - off[r]);
        gc[f] = (int)(gc_before(gcbits, gcincl, y) - gc_before(gcbits, gcincl, x));
    }
}
static int frag_of(int c, int p, const long long* rec_first, const int* len, int R, const int* start, bool* beyond)
{
    *beyond = false;
    if (c < 0 || c >= R) return -1;
    *beyond = p > len[c];
    if (p < 1) return -1;
    int f = -1;
    for (long long k = rec_first[c]; k < rec_first[c + 1]; k++)
        if (start[k] <= p - 1) f = (int)k;
    return f;
}
static void model_assign(void** a, dim3, dim3)
{
    const int *c1 = *(const int**)a[0], *p1 = *(const int**)a[1], *c2 = *(const int**)a[2], *p2 = *(const int**)a[3];
    const long long n = *(long long*)a[4];
    const long long* rec_first = *(const long long**)a[5];
    const int* len = *(const int**)a[6];
    const int R = *(int*)a[7];
    const int* start = *(const int**)a[8];
    int2* store = *(int2**)a[9];
    u64* cursor = *(u64**)a[10];
    const u64 cap = *(u64*)a[11];
    u64* sc = *(u64**)a[12];
    for (long long k = 0; k < n - (g_lose_a_pair ? 1 : 0); k++) {
        bool bx, by;
        const int x = frag_of(c1[k], p1[k], rec_first, len, R, start, &bx), y = frag_of(c2[k], p2[k], rec_first, len, R, start, &by);
        sc[0]++, sc[x < 0 ? 2 : y < 0 ? 3 : 1]++, sc[4] += (u64)bx + (u64)by;
        if (x < 0 || y < 0) continue;
        const u64 slot = (*cursor)++;
        if (slot < cap) store[slot] = int2{std::min(x, y), std::max(x, y)};
    }
}
template <bool SCATTER>
static void model_emit(void** a, dim3, dim3)
{
    const int2* store = *(const int2**)a[0];
    const long long n = *(long long*)a[1];
    const int U = *(int*)a[2];
    u64 *counter = *(u64**)a[3], *ent = *(u64**)a[4];
    const u64 n_ent = *(u64*)a[5];
    u64* sc = *(u64**)a[6];
    for (long long k = 0; k < n; k++) {
        const int2 e = store[k];
        if (e.x < 0 || e.y < e.x || e.y >= U) {
            if (!SCATTER) sc[1]++;
            continue;
        }
        const u64 slot = counter[e.x]++;
        if (!SCATTER) sc[0]++;
        else if (slot < n_ent) ent[slot] = ((u64)(unsigned)e.y << 32) | 1ull;
    }
}
// the row builder's kernels, as tests/sanitize/pairs_harness.cpp models them; the reduction here sums the equal columns for real
static void model_scan_apply(void** a, dim3 grid, dim3)
{
    const u64* in = *(const u64**)a[0];
    u64* out = *(u64**)a[1];
    const long long stride = *(long long*)a[2];
    const int n = *(int*)a[3];
    for (unsigned y = 0; y < grid.y; y++) {
        u64 run = 0;
        for (int i = 0; i < n; i++) out[y * stride + i] = run += in[y * stride + i];
    }
}
template <bool FILL>
static void model_classify(void** a, dim3, dim3)
{
    const u64* rowstart = *(const u64**)a[0];
    const int U = *(int*)a[1], short_max = *(int*)a[2], lds_max = *(int*)a[3];
    u64 *cls = *(u64**)a[4], *cur = *(u64**)a[5];
    int* short_rows = *(int**)a[6];
    Item *lds_items = *(Item**)a[7], *run_items = *(Item**)a[8];
    Long* long_rows = *(Long**)a[9];
    for (int r = 0; r < U; r++) {
        const u64 b = rowstart[r], len = rowstart[r + 1] - b;
        if (len < 2) continue;
        if (len <= (u64)short_max) {
            if (!FILL) cls[0]++, cls[1] += len;
            else short_rows[cur[0]++] = r;
        } else if (len <= (u64)lds_max) {
            if (!FILL) cls[2]++, cls[3] += len;
            else lds_items[cur[1]++] = Item{(long long)b, (int)len, 0};
        } else {
            const u64 run = (u64)lds_max, n_runs = run > 1 ? (len + run - 1) / run : 0;
            if (!FILL) {
                cls[4]++, cls[5] += len, cls[6] += n_runs;
                cls[7] = std::max(cls[7], len);
            } else {
                long_rows[cur[2]++] = Long{(long long)b, (long long)cur[3], (long long)len};
                cur[3] += len;
                for (u64 q = 0; q < n_runs; q++) run_items[cur[4]++] = Item{(long long)(b + q * run), (int)std::min(run, len - q * run), 0};
            }
        }
    }
}
static void model_sort_items(void** a, dim3 grid, dim3)
{
    const Item* items = *(const Item**)a[0];
    u64* ent = *(u64**)a[1];
    for (unsigned i = 0; i < grid.x; i++) std::sort(ent + items[i].off, ent + items[i].off + items[i].len);
}
static void model_sort_wave(void** a, dim3, dim3)
{
    const int* rows = *(const int**)a[0];
    const int n_rows = *(int*)a[1];
    const u64* rowstart = *(const u64**)a[2];
    u64* ent = *(u64**)a[3];
    for (int i = 0; i < n_rows; i++) std::sort(ent + rowstart[rows[i]], ent + rowstart[rows[i] + 1]);
}
static void model_merge(void** a, dim3 grid, dim3) // (the runs are sorted; the merge of a long row is a sort of the whole row here)
{
    const Long* rows = *(const Long**)a[0];
    u64 *ent = *(u64**)a[1], *scratch = *(u64**)a[2];
    const int to_scratch = *(int*)a[4];
    for (unsigned i = 0; i < grid.x; i++) {
        std::sort(ent + rows[i].off, ent + rows[i].off + rows[i].len);
        for (long long e = 0; e < rows[i].len; e++)
            (to_scratch ? scratch[rows[i].scratch + e] : ent[rows[i].off + e]) = to_scratch ? ent[rows[i].off + e] : scratch[rows[i].scratch + e];
        if (to_scratch) std::memcpy(ent + rows[i].off, scratch + rows[i].scratch, (size_t)rows[i].len * sizeof(u64));
    }
}
static bool is_head(const u64* ent, const u64* rowstart, int U, long long e, int* row)
{
    while (*row + 1 < U && rowstart[*row + 1] <= (u64)e) ++*row;
    return (u64)e == rowstart[*row] || (ent[e] >> 32) != (ent[e - 1] >> 32);
}
static const u64* g_rowstart = nullptr; // (k_lift_head_totals reads the heads from the bits k_lift_row_bits set: the model takes the rows themselves)
static int g_U = 0;
static void model_row_bits(void** a, dim3, dim3)
{
    g_rowstart = *(const u64**)a[0];
    g_U = *(int*)a[1];
}
static void model_head_totals(void** a, dim3 grid, dim3)
{
    const u64* ent = *(const u64**)a[0];
    const long long n = *(long long*)a[2];
    u64 *totals = *(u64**)a[3], *n_heads = *(u64**)a[4];
    if (g_no_heads) return;
    int row = 0;
    for (unsigned b = 0; b < grid.x; b++) totals[b] = 0;
    for (long long e = 0; e < n; e++)
        if (is_head(ent, g_rowstart, g_U, e, &row)) totals[e / 2048]++, ++*n_heads;
}
static void model_reduce(void** a, dim3, dim3)
{
    const u64* ent = *(const u64**)a[0];
    const long long n = *(long long*)a[2];
    const u64* rowstart = *(const u64**)a[4];
    const int U = *(int*)a[5];
    const u64 n_out = *(u64*)a[6];
    int* out_col = *(int**)a[7];
    u64 *out_cnt = *(u64**)a[8], *row_heads = *(u64**)a[9];
    int row = 0;
    long long o = -1;
    for (long long e = 0; e < n; e++) {
        if (is_head(ent, rowstart, U, e, &row)) {
            o++;
            if ((u64)o < n_out) out_col[o] = (int)(ent[e] >> 32), row_heads[row]++;
        }
        if (o >= 0 && (u64)o < n_out) out_cnt[o] += ent[e] & 0xffffffffull;
    }
}

// ---- the genome of the harness and its digest by brute force
struct Genome {
    std::vector<std::string> rec;
    std::vector<uint8_t> buf;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    Genome()
    {
        unsigned x = 2024u;
        auto next = [&] { return (x = x * 1664525u + 1013904223u) >> 8; };
        for (int n : {1, 3, 15, 16, 17, 63, 64, 65, 300, 4, 1029}) {
            std::string s((size_t)n, 'A');
            for (char& ch : s) ch = "ACGTacgtGATCGANTCnR"[next() % 19];
            rec.push_back(s);
        }
        rec[9] = "GATC";
        for (const std::string& s : rec) {
            off.push_back((int64_t)buf.size());
            len.push_back((int32_t)s.size());
            buf.insert(buf.end(), s.begin(), s.end());
            buf.push_back(0);
        }
    }
    int R() const { return (int)rec.size(); }
    int begin(ig_ctx* c) const { return ig_pre_begin(c, buf.data(), (int64_t)buf.size(), off.data(), len.data(), R()); }
};
struct Enzymes {
    std::vector<int32_t> len = {4, 5, 16}, cut = {0, 1, 16};
    std::vector<uint8_t> masks;
    Enzymes() : masks(3 * 16, 0)
    {
        const uint8_t gatc[4] = {4, 1, 8, 2}, gantc[5] = {4, 1, 16, 8, 2};
        std::memcpy(&masks[0], gatc, 4);
        std::memcpy(&masks[16], gantc, 5);
        std::memset(&masks[32], 16, 16); // sixteen N: every window of sixteen letters, the cut behind it
    }
    int digest(ig_ctx* c, std::vector<int64_t>& per, int64_t* n_frags, float* ms = nullptr) const
    {
        return ig_pre_digest(c, 3, len.data(), cut.data(), masks.data(), per.data(), n_frags, ms);
    }
};
struct Frag {
    int rec, start, end, gc;
    bool operator==(const Frag& o) const { return rec == o.rec && start == o.start && end == o.end && gc == o.gc; }
};
static std::vector<Frag> brute_digest(const Genome& g, const Enzymes& z)
{
    std::vector<Frag> out;
    for (int r = 0; r < g.R(); r++) {
        const std::string& s = g.rec[(size_t)r];
        const int n = (int)s.size();
        std::set<int> cuts = {0, n};
        for (int e = 0; e < 3; e++)
            for (int at = 0; at + z.len[(size_t)e] <= n; at++) {
                bool ok = true;
                for (int j = 0; j < z.len[(size_t)e]; j++) ok = ok && (code_of((unsigned char)s[(size_t)(at + j)]) & z.masks[(size_t)(16 * e + j)]);
                if (ok) cuts.insert(at + z.cut[(size_t)e]);
            }
        for (auto it = cuts.begin(); std::next(it) != cuts.end(); ++it) {
            int gc = 0;
            for (int k = *it; k < *std::next(it); k++) gc += std::strchr("GCgc", s[(size_t)k]) != nullptr;
            out.push_back(Frag{r, *it, *std::next(it), gc});
        }
    }
    return out;
}
static int fetch_fragments(ig_ctx* c, int64_t n, int64_t piece, std::vector<Frag>& out)
{
    out.clear();
    for (int64_t a = 0; a < n; a += piece) {
        const int64_t m = std::min(piece, n - a);
        std::vector<int32_t> rec((size_t)m + 1, -7), st((size_t)m + 1, -7), en((size_t)m + 1, -7), gc((size_t)m + 1, -7);
        CHECK(ig_pre_fragments(c, a, m, rec.data(), st.data(), en.data(), gc.data()) == 0 && rec[(size_t)m] == -7 && gc[(size_t)m] == -7);
        for (int64_t k = 0; k < m; k++) out.push_back(Frag{rec[(size_t)k], st[(size_t)k], en[(size_t)k], gc[(size_t)k]});
    }
    return 0;
}

struct Chunk {
    std::vector<int32_t> c1, p1, c2, p2;
    int64_t sc[8];
    Chunk(int n, int seed, const Genome& g) : c1((size_t)n), p1((size_t)n), c2((size_t)n), p2((size_t)n)
    {
        unsigned x = 777u + (unsigned)seed;
        auto next = [&] { return (x = x * 1664525u + 1013904223u) >> 8; };
        for (int k = 0; k < n; k++) {
            c1[(size_t)k] = (int32_t)(next() % (unsigned)(g.R() + 1)) - (next() % 40 == 0);
            c2[(size_t)k] = next() % 3 ? c1[(size_t)k] : (int32_t)(next() % (unsigned)(g.R() + 1));
            p1[(size_t)k] = (int32_t)(next() % 1100), p2[(size_t)k] = next() % 2 ? p1[(size_t)k] + (int32_t)(next() % 9) : (int32_t)(next() % 1100);
        }
        for (int k = 0; k < 8; k++) sc[k] = -7;
    }
    int add(ig_ctx* c, float* ms = nullptr)
    {
        for (int k = 0; k < 8; k++) sc[k] = -7;
        return ig_pre_add_pairs(c, c1.data(), p1.data(), c2.data(), p2.data(), (int64_t)c1.size(), sc, ms);
    }
};
// the pixels against a dense brute force over the fetched fragments
static int pixels_agree(ig_ctx* c, const std::vector<Frag>& frags, const Genome& g, const std::vector<const Chunk*>& chunks)
{
    const int U = (int)frags.size();
    std::vector<int64_t> dense((size_t)U * (size_t)U, 0);
    std::vector<long long> first((size_t)g.R() + 1, 0);
    std::vector<int> start;
    for (const Frag& f : frags) first[(size_t)f.rec + 1]++, start.push_back(f.start);
    for (int r = 0; r < g.R(); r++) first[(size_t)r + 1] += first[(size_t)r];
    int64_t want[5] = {0, 0, 0, 0, 0};
    for (const Chunk* ch : chunks)
        for (size_t k = 0; k < ch->c1.size(); k++) {
            bool bx, by;
            const int x = frag_of(ch->c1[k], ch->p1[k], first.data(), g.len.data(), g.R(), start.data(), &bx), y = frag_of(ch->c2[k], ch->p2[k], first.data(), g.len.data(), g.R(), start.data(), &by);
            want[0]++, want[x < 0 ? 2 : y < 0 ? 3 : 1]++, want[4] += bx + by;
            if (x >= 0 && y >= 0) dense[(size_t)std::min(x, y) * (size_t)U + (size_t)std::max(x, y)]++;
        }
    int64_t E = -7, sc[8];
    std::vector<float> ms(7, -7.0f);
    CHECK(ig_pre_pixels_build(c, &E, sc, ms.data()) == 0 && E >= 0 && ms[6] != -7.0f);
    for (int k = 0; k < 5; k++) CHECK(sc[k] == want[k]);
    CHECK(sc[5] == E && sc[6] == U && sc[7] == want[1] && sc[0] == sc[1] + sc[2] + sc[3]);
    std::vector<int64_t> rowptr((size_t)U + 2, -7), count((size_t)E + 1, -7);
    std::vector<int32_t> col((size_t)E + 1, -7);
    CHECK(ig_pre_pixels_rows(c, rowptr.data(), U) != 0 && rowptr[0] == -7);
    CHECK(ig_pre_pixels_rows(c, rowptr.data(), U + 1) == 0 && rowptr[0] == 0 && rowptr[(size_t)U] == E && rowptr[(size_t)U + 1] == -7);
    for (int64_t a = 0; a < E; a += 7) CHECK(ig_pre_pixels_fetch(c, a, std::min<int64_t>(7, E - a), col.data() + a, count.data() + a) == 0);
    CHECK(col[(size_t)E] == -7 && count[(size_t)E] == -7 && ig_pre_pixels_fetch(c, E, 1, col.data(), count.data()) != 0 && ig_pre_pixels_fetch(c, 0, 0, nullptr, nullptr) == 0);
    int64_t nz = 0;
    for (int64_t v : dense) nz += v != 0;
    CHECK(nz == E);
    for (int u = 0; u < U; u++)
        for (int64_t e = rowptr[(size_t)u]; e < rowptr[(size_t)u + 1]; e++) {
            CHECK(col[(size_t)e] >= u && col[(size_t)e] < U && (e == rowptr[(size_t)u] || col[(size_t)e] > col[(size_t)e - 1]));
            CHECK(count[(size_t)e] == dense[(size_t)u * (size_t)U + (size_t)col[(size_t)e]]);
        }
    return 0;
}

// ---- a genome beyond 2^32 bytes: two records of 2^31 - 648 bases in front, so that the third straddles the coordinate 2^32 and the
// fourth lies behind it; every base an A but for a site GATC at chosen places, one of them across 2^32 itself (which is also a bitmap
// word's and a run's boundary).  The 64-bit offsets of ig_pre_begin, its upload in pieces, the sizes of the padded sequence and of the
// bitmaps, and the coordinates the models of k_pre_marks, k_pre_cuts, k_pre_frags and the G+C prefix read are all beyond 32 bits.
static int beyond_4gib()
{
    const int64_t L = 2147483000;
    const std::vector<int32_t> len = {(int32_t)L, (int32_t)L, 10000, 5000};
    std::vector<int64_t> off;
    int64_t at = 0;
    for (int32_t n : len) off.push_back(at), at += (int64_t)n + 1;
    const int64_t two32 = (int64_t)1 << 32;
    CHECK(off[2] < two32 && off[2] + len[2] > two32 && off[3] > two32 && at > two32);
    std::vector<uint8_t> buf((size_t)at, (uint8_t)'A');
    for (size_t r = 0; r < 4; r++) buf[(size_t)(off[r] + len[r])] = 0;
    const int64_t across = two32 - 2 - off[2]; // the site's four letters lie on the coordinates 2^32 - 2 .. 2^32 + 1
    const std::vector<std::pair<int, int64_t>> sites = {{0, 0}, {1, L - 4}, {2, 1200}, {2, across}, {2, 1400}, {3, 100}, {3, 4996}};
    for (const auto& s : sites) std::memcpy(&buf[(size_t)(off[(size_t)s.first] + s.second)], "GATC", 4);
    const std::vector<Frag> want = {{0, 0, (int)L, 2}, {1, 0, (int)L - 4, 0}, {1, (int)L - 4, (int)L, 2}, {2, 0, 1200, 0}, {2, 1200, (int)across, 2}, {2, (int)across, 1400, 2},
                                    {2, 1400, 10000, 2}, {3, 0, 100, 0}, {3, 100, 4996, 2}, {3, 4996, 5000, 2}};
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0);
    std::vector<int64_t> bad = off;
    bad[3] -= two32; // an offset that lost its upper half is refused on the host
    CHECK(ig_pre_begin(c, buf.data(), at, bad.data(), len.data(), 4) != 0 && std::strstr(ig_last_error(), "record 3 starts at"));
    g_free_bytes = (size_t)1 << 32; // less than the sequence alone
    CHECK(ig_pre_begin(c, buf.data(), at, off.data(), len.data(), 4) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
    g_free_bytes = (size_t)1 << 34;
    CHECK(ig_pre_begin(c, buf.data(), at, off.data(), len.data(), 4) == 0);
    const int32_t site_len = 4, cut = 0;
    uint8_t masks[16] = {4, 1, 8, 2};
    int64_t per[5] = {-7, -7, -7, -7, -7}, n_frags = -7;
    CHECK(ig_pre_digest(c, 1, &site_len, &cut, masks, per, &n_frags, nullptr) == 0);
    CHECK(n_frags == 10 && per[0] == 1 && per[1] == 2 && per[2] == 4 && per[3] == 3 && per[4] == -7);
    std::vector<Frag> got;
    CHECK(fetch_fragments(c, n_frags, 3, got) == 0 && got == want);
    // pair ends on either side of 2^32 and in the record behind it; a position beyond the longest record
    const int32_t c1[4] = {2, 2, 3, 0}, p1[4] = {(int32_t)across, (int32_t)across + 1, 101, 0x7fffffff}, c2[4] = {3, 2, 3, 1}, p2[4] = {4997, 1401, 100, (int32_t)L - 3};
    int64_t sc[8], E = -7, rowptr[11], count[4];
    int32_t col[4];
    CHECK(ig_pre_add_pairs(c, c1, p1, c2, p2, 4, sc, nullptr) == 0 && sc[0] == 4 && sc[1] == 4 && sc[4] == 1 && sc[5] == 4);
    CHECK(ig_pre_pixels_build(c, &E, sc, nullptr) == 0 && E == 4 && sc[6] == 10);
    CHECK(ig_pre_pixels_rows(c, rowptr, 11) == 0 && ig_pre_pixels_fetch(c, 0, 4, col, count) == 0);
    const int64_t want_rows[11] = {0, 1, 1, 1, 1, 2, 3, 3, 4, 4, 4};
    const int32_t want_col[4] = {2, 9, 6, 8}; // (0, 2): the last base of record 0 with record 1's tail; (4, 9); (5, 6); (7, 8)
    for (int k = 0; k < 11; k++) CHECK(rowptr[k] == want_rows[k]);
    for (int k = 0; k < 4; k++) CHECK(col[k] == want_col[k] && count[k] == 1);
    ig_destroy(c); // a live session of 4 GiB in front of ig_destroy
    return 0;
}

int main()
{
    fake_hip::set_model("k_pre_sites", model_sites);
    fake_hip::set_model("k_pre_marks", model_marks);
    fake_hip::set_model("k_pre_popc", model_popc);
    fake_hip::set_model("k_pre_cuts", model_cuts);
    fake_hip::set_model("k_pre_frags", model_frags);
    fake_hip::set_model("k_pre_assign", model_assign);
    fake_hip::set_model("k_pre_emitILb0E", model_emit<false>);
    fake_hip::set_model("k_pre_emitILb1E", model_emit<true>);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_row_bits", model_row_bits);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_lift_reduce", model_reduce);

    const Fixture fx;
    const Genome g;
    const Enzymes z;
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    std::vector<int64_t> per((size_t)g.R() + 1, -7);
    int64_t n_frags = -7;
    Chunk small(5, 1, g), mid(70, 2, g), big(900, 3, g);

    // ---- nothing without a session
    CHECK(ig_pre_end(c) != 0 && std::strstr(ig_last_error(), "no session"));
    CHECK(ig_pre_clear(c) != 0 && std::strstr(ig_last_error(), "no session"));
    CHECK(z.digest(c, per, &n_frags) != 0 && std::strstr(ig_last_error(), "no session") && per[0] == -7 && n_frags == -7);
    CHECK(small.add(c) != 0 && std::strstr(ig_last_error(), "no session") && small.sc[0] == -7);
    {
        int64_t E = -7, sc[8] = {-7};
        CHECK(ig_pre_pixels_build(c, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "no session") && E == -7 && sc[0] == -7);
    }

    // ---- the refusals of the records: on the host, before any device work
    {
        const long before = fake_hip::allocations();
        Genome t = g;
        t.buf[(size_t)t.off[5] + 2] = 'X';
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "record 5, position 3") && std::strstr(ig_last_error(), "0x58"));
        t = g, t.buf[(size_t)t.off[8] + 10] = 0; // a zero byte inside a record is no separator
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "record 8, position 11"));
        t = g, t.buf[(size_t)t.off[1] - 1] = 'A';
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "behind record 0"));
        t = g, t.off[3] += 1;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "record 3 starts at"));
        t = g, t.len[2] = 0;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "record 2 is empty"));
        t = g, t.len[10] += 1;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "record 10 ends at"));
        CHECK(ig_pre_begin(c, g.buf.data(), (int64_t)g.buf.size() + 1, g.off.data(), g.len.data(), g.R()) != 0 && std::strstr(ig_last_error(), "bytes, not"));
        CHECK(ig_pre_begin(c, nullptr, (int64_t)g.buf.size(), g.off.data(), g.len.data(), g.R()) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_pre_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), 0) != 0 && std::strstr(ig_last_error(), "bad sizes"));
        g_free_bytes = 1024;
        CHECK(g.begin(c) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
        g_free_bytes = (size_t)1 << 34;
        CHECK(fake_hip::allocations() == before); // none of them reached the device
        CHECK(ig_pre_end(c) != 0);                // none of them left a session
    }

    // ---- begin twice; nothing before a digest; the refusals of the sites; the digest against the brute force, fetched in pieces
    CHECK(g.begin(c) == 0);
    CHECK(g.begin(c) != 0 && std::strstr(ig_last_error(), "a session is open"));
    CHECK(small.add(c) != 0 && std::strstr(ig_last_error(), "nothing is digested") && small.sc[0] == -7);
    {
        int32_t rec = -7;
        int64_t E = -7, sc[8] = {-7};
        CHECK(ig_pre_fragments(c, 0, 1, &rec, &rec, &rec, &rec) != 0 && std::strstr(ig_last_error(), "nothing is digested") && rec == -7);
        CHECK(ig_pre_pixels_build(c, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "nothing is digested") && E == -7);
        Enzymes bad = z;
        bad.len[1] = 17;
        CHECK(bad.digest(c, per, &n_frags) != 0 && std::strstr(ig_last_error(), "17 letters") && n_frags == -7);
        bad = z, bad.cut[0] = 5;
        CHECK(bad.digest(c, per, &n_frags) != 0 && std::strstr(ig_last_error(), "cuts behind 5 of 4"));
        bad = z, bad.masks[17] = 0;
        CHECK(bad.digest(c, per, &n_frags) != 0 && std::strstr(ig_last_error(), "enzyme 1, letter 1"));
        bad = z, bad.masks[2] = 17;
        CHECK(bad.digest(c, per, &n_frags) != 0 && std::strstr(ig_last_error(), "enzyme 0, letter 2") && per[0] == -7);
        CHECK(ig_pre_digest(c, 5, z.len.data(), z.cut.data(), z.masks.data(), per.data(), &n_frags, nullptr) != 0 && std::strstr(ig_last_error(), "1 .. 4 enzymes"));
        CHECK(ig_pre_digest(c, 3, z.len.data(), z.cut.data(), nullptr, per.data(), &n_frags, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
        g_lose_a_cut = true; // fewer cuts than two per record: a device error the host catches, nothing digested
        CHECK(z.digest(c, per, &n_frags) != 0 && std::strstr(ig_last_error(), "device error") && n_frags == -7);
        CHECK(ig_pre_fragments(c, 0, 1, &rec, &rec, &rec, &rec) != 0 && rec == -7);
        g_lose_a_cut = false;
    }
    const std::vector<Frag> want = brute_digest(g, z);
    std::vector<Frag> frags;
    std::vector<float> ms(4, -7.0f);
    CHECK(z.digest(c, per, &n_frags, ms.data()) == 0 && n_frags == (int64_t)want.size() && per[(size_t)g.R()] == -7 && ms[3] != -7.0f);
    CHECK(fetch_fragments(c, n_frags, 13, frags) == 0 && frags == want);
    CHECK(fetch_fragments(c, n_frags, n_frags, frags) == 0 && frags == want && (int64_t)want.size() > 3 * g.R());
    {
        int64_t total = 0;
        for (int r = 0; r < g.R(); r++) total += per[(size_t)r];
        int32_t rec = -7;
        CHECK(total == n_frags && per[0] == 1 && per[9] == 1);
        CHECK(ig_pre_fragments(c, n_frags, 1, &rec, &rec, &rec, &rec) != 0 && ig_pre_fragments(c, -1, 1, &rec, &rec, &rec, &rec) != 0 && rec == -7);
        CHECK(ig_pre_fragments(c, 0, 1, nullptr, &rec, &rec, &rec) != 0 && std::strstr(ig_last_error(), "NULL") && ig_pre_fragments(c, n_frags, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    }

    // ---- an empty store; the store grows across the chunks; the pixels behind every chunk, under the default and lowered limits
    CHECK(pixels_agree(c, frags, g, {}) == 0);
    {
        std::vector<const Chunk*> seen;
        int64_t stored = 0;
        for (Chunk* ch : {&small, &mid, &big, &small}) {
            float t = -7.0f;
            CHECK(ch->add(c, &t) == 0 && ch->sc[5] == stored + ch->sc[1] && ch->sc[0] == (int64_t)ch->c1.size() && t != -7.0f);
            stored = ch->sc[5];
            seen.push_back(ch);
            CHECK(pixels_agree(c, frags, g, seen) == 0);
        }
        CHECK(stored > 100);
        CHECK(ig_debug_assembly_contacts_limits(c, 2, 4) == 0 && pixels_agree(c, frags, g, seen) == 0 && ig_debug_assembly_contacts_limits(c, 0, 0) == 0);
        int64_t sc[8] = {-7};
        CHECK(ig_pre_add_pairs(c, nullptr, nullptr, nullptr, nullptr, 0, sc, nullptr) == 0 && sc[0] == 0 && sc[5] == stored); // an empty chunk
        sc[0] = -7;
        CHECK(ig_pre_add_pairs(c, small.c1.data(), small.p1.data(), small.c2.data(), small.p2.data(), -1, sc, nullptr) != 0 && sc[0] == -7);
        CHECK(ig_pre_add_pairs(c, nullptr, small.p1.data(), small.c2.data(), small.p2.data(), 5, sc, nullptr) != 0 && sc[0] == -7);
        CHECK(ig_pre_add_pairs(c, small.c1.data(), small.p1.data(), small.c2.data(), small.p2.data(), 5, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(pixels_agree(c, frags, g, seen) == 0);
        // the device errors and the free-memory guards: each leaves the store as it was and nothing to fetch
        int64_t E = -7;
        std::vector<int64_t> rowptr((size_t)n_frags + 1, -7);
        g_no_heads = true;
        CHECK(ig_pre_pixels_build(c, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "distinct") && E == -7);
        CHECK(ig_pre_pixels_rows(c, rowptr.data(), n_frags + 1) != 0 && std::strstr(ig_last_error(), "nothing is built") && rowptr[0] == -7);
        g_no_heads = false;
        g_free_bytes = 4096;
        CHECK(ig_pre_pixels_build(c, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && E == -7);
        Chunk huge(5000, 4, g);
        CHECK(huge.add(c) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && huge.sc[0] == -7);
        g_free_bytes = (size_t)1 << 34;
        g_lose_a_pair = true;
        CHECK(mid.add(c) != 0 && std::strstr(ig_last_error(), "device error") && mid.sc[0] == -7);
        g_lose_a_pair = false;
        CHECK(pixels_agree(c, frags, g, seen) == 0);
        // clear: the store is empty, the digest stays; a second digest empties the store too
        CHECK(ig_pre_clear(c) == 0 && pixels_agree(c, frags, g, {}) == 0 && big.add(c) == 0 && big.sc[5] == big.sc[1] && pixels_agree(c, frags, g, {&big}) == 0);
        CHECK(z.digest(c, per, &n_frags) == 0 && fetch_fragments(c, n_frags, 50, frags) == 0 && frags == want && pixels_agree(c, frags, g, {}) == 0);
    }
    CHECK(ig_pre_end(c) == 0 && ig_pre_end(c) != 0 && std::strstr(ig_last_error(), "no session"));

    // ---- every allocation of a session fails once: an error that names hipMalloc, nothing leaked, and the next session works
    {
        Chunk a(700, 5, g), b(40, 6, g);
        const auto session = [&]() -> int {
            (void)ig_pre_end(c); // (whatever the turn before left open)
            int rc = g.begin(c);
            if (!rc) rc = z.digest(c, per, &n_frags);
            if (!rc) rc = b.add(c);
            if (!rc) rc = a.add(c); // the store grows, the staging arrays too
            int64_t E, sc[8];
            if (!rc) rc = ig_pre_pixels_build(c, &E, sc, nullptr);
            return rc;
        };
        if (allocation_failure_sweep(fx, c, 120, 60, 40, 30, session, [&] { return true; }, [&] { return session() == 0 && pixels_agree(c, frags, g, {&b, &a}) == 0; })) return 1;
    }

    // ---- a failed chunk in front of ig_destroy; a live session with built pixels in front of ig_destroy
    (void)ig_pre_end(c);
    CHECK(g.begin(c) == 0 && z.digest(c, per, &n_frags) == 0 && small.add(c) == 0);
    CHECK(failed_call_before_destroy(c, 0, [&] { return big.add(c); }) != 0);
    CHECK(ig_create(0, &c) == 0 && g.begin(c) == 0 && z.digest(c, per, &n_frags) == 0 && big.add(c) == 0 && pixels_agree(c, frags, g, {&big}) == 0);
    ig_destroy(c);
    if (beyond_4gib()) return 1;
    std::printf("pre harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
