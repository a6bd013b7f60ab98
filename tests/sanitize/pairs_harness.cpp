// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the read pairs lifted onto the current genome
// (csrc/ig_host_pairs.inc: the session, the store and its growth, the staging of a chunk, the pixels through the row builder into the
// assembly-contacts snapshot, the histogram) with the sort and reduction it shares with the other reports (csrc/ig_host_rows.inc): a
// stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is
// checked against the real allocation sizes).  The models below do what the three kernels do, word for word, so the sizes of the table,
// of the store behind every growth and of the staging arrays are all exercised; memory safety, the lifetime of the session and every
// refusal are the subject.  Built and run by tests/test_pairs_lift_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_rows.cuh, ig_kernels_pairs.cuh: device code, not included here)
struct Item {
    long long off;
    int len, pad;
};
struct Long {
    long long off, scratch, len;
};
struct Iv {
    int src_end, new_start, scaf_rev, position;
};
struct Out {
    int *scaffold1, *pos1, *unit1, *scaffold2, *pos2, *unit2;
    unsigned char *rev1, *rev2, *status;
};
struct Store {
    int4* ends;
    int2* unit;
    unsigned char* flag;
};

static bool g_no_heads = false;
static bool g_lose_a_pair = false; // the lift counts a pair less than it was given: a device error the host must catch
static size_t g_free_bytes = (size_t)1 << 34;
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

struct End {
    bool hit;
    int scaffold, new0, unit, rev;
};
static End lift_end(int c, int p, const int* rowptr, int n_contigs, const int* start, const Iv* iv)
{
    End e = {false, -1, 0, -1, 0};
    if (c < 0 || c >= n_contigs || p < 1) return e;
    int i = -1;
    for (int k = rowptr[c]; k < rowptr[c + 1]; k++)
        if (start[k] <= p - 1) i = k;
    if (i < 0 || p - 1 >= iv[i].src_end) return e;
    e.hit = true;
    if (iv[i].scaf_rev < 0) return e;
    const int off = p - 1 - start[i];
    e.rev = iv[i].scaf_rev & 1, e.scaffold = iv[i].scaf_rev >> 1, e.unit = iv[i].position;
    e.new0 = iv[i].new_start + (e.rev ? iv[i].src_end - start[i] - 1 - off : off);
    return e;
}
static void model_lift(void** a, dim3, dim3)
{
    const int *c1 = *(const int**)a[0], *p1 = *(const int**)a[1], *c2 = *(const int**)a[2], *p2 = *(const int**)a[3];
    const unsigned char* strands = *(const unsigned char**)a[4];
    const long long n = *(long long*)a[5];
    const int* rowptr = *(const int**)a[6];
    const int n_contigs = *(int*)a[7];
    const int* start = *(const int**)a[8];
    const Iv* iv = *(const Iv**)a[9];
    const Out out = *(Out*)a[10];
    const Store st = *(Store*)a[11];
    u64* cursor = *(u64**)a[12];
    const u64 cap = *(u64*)a[13];
    u64* sc = *(u64**)a[14];
    for (long long k = 0; k < n - (g_lose_a_pair ? 1 : 0); k++) {
        const End x = lift_end(c1[k], p1[k], rowptr, n_contigs, start, iv), y = lift_end(c2[k], p2[k], rowptr, n_contigs, start, iv);
        const int status = !x.hit ? 1 : !y.hit ? 2 : (x.scaffold < 0 || y.scaffold < 0) ? 3 : 0;
        if (out.status) {
            out.scaffold1[k] = x.scaffold, out.pos1[k] = x.scaffold < 0 ? 0 : x.new0 + 1, out.unit1[k] = x.unit, out.rev1[k] = (unsigned char)x.rev;
            out.scaffold2[k] = y.scaffold, out.pos2[k] = y.scaffold < 0 ? 0 : y.new0 + 1, out.unit2[k] = y.unit, out.rev2[k] = (unsigned char)y.rev;
            out.status[k] = (unsigned char)status;
        }
        sc[0]++, sc[1 + status]++;
        if (status) continue;
        const u64 slot = (*cursor)++;
        if (slot >= cap) continue;
        const int sb = strands ? strands[k] : 0;
        st.ends[slot] = int4{x.scaffold, x.new0, y.scaffold, y.new0};
        st.unit[slot] = int2{x.unit, y.unit};
        st.flag[slot] = (unsigned char)((x.rev ? 1 : 0) | (y.rev ? 2 : 0) | ((sb & 1) ? 4 : 0) | ((sb & 2) ? 8 : 0));
    }
}
static int unit_of(int kind, unsigned binsize, const int* tab, int scaffold, int new0, int position)
{
    return kind == 0 ? position : kind == 1 ? tab[position] : kind == 3 ? scaffold : tab[scaffold] + (int)((unsigned)new0 / binsize);
}
template <bool SCATTER>
static void model_emit(void** a, dim3, dim3)
{
    const Store st = *(Store*)a[0];
    const long long n = *(long long*)a[1];
    const int kind = *(int*)a[2];
    const unsigned binsize = *(unsigned*)a[3];
    const int* tab = *(const int**)a[4];
    const int U = *(int*)a[5];
    u64 *counter = *(u64**)a[6], *ent = *(u64**)a[7];
    const u64 n_ent = *(u64*)a[8];
    u64* sc = *(u64**)a[9];
    for (long long k = 0; k < n; k++) {
        const int4 e = st.ends[k];
        const int2 u = st.unit[k];
        const int x = unit_of(kind, binsize, tab, e.x, e.y, u.x), y = unit_of(kind, binsize, tab, e.z, e.w, u.y);
        if (x < 0 || y < 0 || x >= U || y >= U) {
            if (!SCATTER) sc[1]++;
            continue;
        }
        const u64 slot = counter[std::min(x, y)]++;
        if (!SCATTER) sc[0]++;
        else if (slot < n_ent) ent[slot] = ((u64)(unsigned)std::max(x, y) << 32) | 1ull;
    }
}
static void model_law(void** a, dim3, dim3)
{
    const Store st = *(Store*)a[0];
    const long long n = *(long long*)a[1];
    const long long* edges = *(const long long**)a[2];
    const int n_edges = *(int*)a[3], flip = *(int*)a[4];
    u64* counts = *(u64**)a[5];
    for (long long k = 0; k < n; k++) {
        const int4 e = st.ends[k];
        if (e.x != e.z) continue;
        const int f = st.flag[k];
        int s1 = (f >> 2) & 1, s2 = (f >> 3) & 1, idx = -1;
        if (flip) s1 ^= f & 1, s2 ^= (f >> 1) & 1;
        const long long d = std::llabs((long long)e.w - e.y);
        for (int q = 0; q < n_edges; q++)
            if (edges[q] <= d) idx = q;
        counts[(s1 * 2 + s2) * (n_edges - 1) + std::min(std::max(idx, 0), n_edges - 2)]++;
    }
}
// the row builder's kernels, as tests/sanitize/zoom_harness.cpp models them
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
static void model_merge(void** a, dim3 grid, dim3)
{
    const Long* rows = *(const Long**)a[0];
    u64 *ent = *(u64**)a[1], *scratch = *(u64**)a[2];
    const int to_scratch = *(int*)a[4];
    for (unsigned i = 0; i < grid.x; i++)
        for (long long e = 0; e < rows[i].len; e++)
            (to_scratch ? scratch[rows[i].scratch + e] : ent[rows[i].off + e]) = to_scratch ? ent[rows[i].off + e] : scratch[rows[i].scratch + e];
}
static void model_head_totals(void** a, dim3 grid, dim3)
{
    const long long n = *(long long*)a[2];
    u64 *totals = *(u64**)a[3], *n_heads = *(u64**)a[4];
    if (g_no_heads) return;
    for (unsigned b = 0; b < grid.x; b++) totals[b] = (u64)std::min<long long>(2048, n - 2048ll * b); // every entry is a head
    *n_heads += (u64)n;
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
    for (long long e = 0; e < n && (u64)e < n_out; e++) {
        while (row + 1 < U && rowstart[row + 1] <= (u64)e) row++;
        out_col[e] = (int)(ent[e] >> 32);
        out_cnt[e] += ent[e] & 0xffffffffull;
        row_heads[row]++;
    }
}
static void model_zoom_rowstart(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int* map = *(const int**)a[1];
    const int U = *(int*)a[2], C = *(int*)a[3];
    u64* segstart = *(u64**)a[4];
    for (int u = 0; u <= U; u++) {
        const int prev = u == 0 ? -1 : map[u - 1], cur = u == U ? C : map[u];
        for (int R = prev + 1; R <= cur; R++) segstart[R] = rowptr[u];
    }
}
static void model_zoom_words(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int* col = *(const int**)a[1];
    const int* map = *(const int**)a[2];
    const int U = *(int*)a[3];
    const long long K = *(long long*)a[4];
    const u64* segstart = *(const u64**)a[5];
    u64* word = *(u64**)a[6];
    int u = 0;
    for (long long e = 0; e < K; e++) {
        while (u + 1 < U && rowptr[u + 1] <= (u64)e) u++;
        word[e] = ((u64)(unsigned)map[col[e]] << 32) | ((u64)e - segstart[map[u]]);
    }
}
static void model_zoom_reduce(void** a, dim3, dim3)
{
    const u64* word = *(const u64**)a[0];
    const long long n = *(long long*)a[2];
    const u64* segstart = *(const u64**)a[4];
    const int C = *(int*)a[5];
    const u64* fine_cnt = *(const u64**)a[6];
    const u64 n_out = *(u64*)a[7];
    int* out_col = *(int**)a[8];
    u64 *out_cnt = *(u64**)a[9], *row_heads = *(u64**)a[10];
    int R = 0;
    for (long long e = 0; e < n && (u64)e < n_out; e++) {
        while (R + 1 < C && segstart[R + 1] <= (u64)e) R++;
        out_col[e] = (int)(word[e] >> 32);
        out_cnt[e] += fine_cnt[segstart[R] + (word[e] & 0xffffffffull)];
        row_heads[R]++;
    }
}

// The session's table: contig 0 [0, 10) [10, 11) reversed [15, 30) reversed; contig 1 none; contig 2 [0, 7) unplaced, [7, 20).  Scaffold 0
// (29 bp) holds the intervals 4, 1, 2 in that order, scaffold 1 (10 bp) interval 0: T = 4 positions, one bin each.
struct Table {
    std::vector<int32_t> rowptr = {0, 3, 3, 5}, start = {0, 10, 15, 0, 7}, end = {10, 11, 30, 7, 20}, new_start = {0, 13, 14, 0, 0}, scaffold = {1, 0, 0, -1, 0},
                         position = {3, 1, 2, -1, 0}, bin_unit = {0, 1, 2, 3};
    std::vector<uint8_t> reversed = {0, 1, 1, 0, 0};
    std::vector<int64_t> len = {29, 10};
    int64_t reserve = 1;
    int begin(ig_ctx* c) const
    {
        return ig_pairs_begin(c, rowptr.data(), (int32_t)rowptr.size() - 1, start.data(), end.data(), new_start.data(), scaffold.data(), reversed.data(), position.data(),
                              (int64_t)start.size(), len.data(), (int32_t)len.size(), bin_unit.data(), (int64_t)bin_unit.size(), 4, reserve);
    }
};

struct Chunk {
    std::vector<int32_t> c1, p1, c2, p2, s1, q1, u1, s2, q2, u2;
    std::vector<uint8_t> strands, r1, r2, status;
    int64_t sc[8];
    explicit Chunk(int n, int seed) : c1((size_t)n), p1((size_t)n), c2((size_t)n), p2((size_t)n), strands((size_t)n)
    {
        unsigned x = 12345u + (unsigned)seed;
        auto next = [&] { return (x = x * 1664525u + 1013904223u) >> 8; };
        for (int k = 0; k < n; k++) {
            c1[(size_t)k] = (int32_t)(next() % 4) - (next() % 50 == 0), p1[(size_t)k] = (int32_t)(next() % 33);
            c2[(size_t)k] = next() % 3 ? c1[(size_t)k] : (int32_t)(next() % 4), p2[(size_t)k] = (int32_t)(next() % 33);
            strands[(size_t)k] = (uint8_t)(next() % 4);
        }
        reset();
    }
    void reset()
    {
        const size_t n = c1.size() + 1; // one word more than the call may write
        for (auto* v : {&s1, &q1, &u1, &s2, &q2, &u2}) v->assign(n, -7);
        for (auto* v : {&r1, &r2, &status}) v->assign(n, 77);
        for (int k = 0; k < 8; k++) sc[k] = -7;
    }
    int lift(ig_ctx* c, bool outputs = true)
    {
        reset();
        const int64_t n = (int64_t)c1.size();
        if (!outputs) return ig_pairs_lift(c, c1.data(), p1.data(), c2.data(), p2.data(), strands.data(), n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sc);
        return ig_pairs_lift(c, c1.data(), p1.data(), c2.data(), p2.data(), strands.data(), n, s1.data(), q1.data(), u1.data(), r1.data(), s2.data(), q2.data(), u2.data(),
                             r2.data(), status.data(), sc);
    }
    bool untouched() const { return sc[0] == -7 && sc[5] == -7 && s1[0] == -7 && status[0] == 77; }
    bool consistent() const
    {
        const size_t n = c1.size();
        int64_t by[4] = {0, 0, 0, 0};
        for (size_t k = 0; k < n; k++) {
            if (status[k] > 3) return false;
            by[status[k]]++;
            if (status[k] == 0 && (s1[k] < 0 || s1[k] > 1 || q1[k] < 1 || q1[k] > (s1[k] ? 10 : 29) || u1[k] < 0 || u1[k] > 3 || q2[k] < 1)) return false;
        }
        return sc[0] == (int64_t)n && sc[1] == by[0] && sc[2] == by[1] && sc[3] == by[2] && sc[4] == by[3] && s1[n] == -7 && status[n] == 77 && r2[n] == 77;
    }
};

static bool nothing_built(ig_ctx* c)
{
    int32_t col = -7;
    int64_t cnt = -7;
    return ig_assembly_contacts_fetch(c, 0, 0, &col, &cnt) != 0 && std::strstr(ig_last_error(), "nothing is built") && col == -7;
}
// the pixels of every kind, fetched whole; a coarsening behind the fixed bins
static int all_pixels(ig_ctx* c, int64_t stored)
{
    const int64_t units[4] = {4, 4, 0, 2};
    for (int kind = 0; kind < 4; kind++)
        for (int64_t B : {(int64_t)1, (int64_t)4, (int64_t)1000}) {
            if (kind != 2 && B != 1) continue;
            int64_t U = -7, E = -7, sc[8];
            CHECK(ig_pairs_pixels_build(c, kind, kind == 2 ? B : 0, &U, &E, sc) == 0);
            const int64_t want_U = kind == 2 ? (29 + B - 1) / B + (10 + B - 1) / B : units[kind];
            CHECK(U == want_U && sc[0] == stored && sc[1] == stored && sc[6] == U && sc[7] == E && E <= stored);
            std::vector<int64_t> rowptr((size_t)U + 2, -7), count((size_t)E + 1, -7);
            std::vector<int32_t> col((size_t)E + 1, -7);
            CHECK(ig_assembly_contacts_rows(c, rowptr.data(), U + 1) == 0 && rowptr[0] == 0 && rowptr[(size_t)U] == E && rowptr[(size_t)U + 1] == -7);
            CHECK(ig_assembly_contacts_fetch(c, 0, E, col.data(), count.data()) == 0 && col[(size_t)E] == -7);
            int64_t total = 0;
            for (int64_t e = 0; e < E; e++) total += count[(size_t)e];
            CHECK(total == stored);
            if (kind == 2 && B == 4) { // 8 + 3 fixed bins -> the two scaffolds
                std::vector<int32_t> map((size_t)U);
                for (int64_t u = 0; u < U; u++) map[(size_t)u] = u < 8 ? 0 : 1;
                int64_t E2 = -7;
                CHECK(ig_assembly_contacts_coarsen(c, map.data(), U, 2, &E2, sc) == 0 && E2 >= 0 && E2 <= E && sc[2] == stored && sc[6] == 2);
            }
        }
    return 0;
}
static int law(ig_ctx* c, int64_t stored)
{
    std::vector<int64_t> edges(512);
    for (int k = 0; k < 512; k++) edges[(size_t)k] = k;
    for (int n_edges : {2, 9, 512})
        for (int flip = 0; flip < 2; flip++) {
            std::vector<int64_t> counts((size_t)4 * (size_t)(n_edges - 1) + 1, -7);
            int64_t sc[8];
            CHECK(ig_pairs_law(c, edges.data(), n_edges, flip, counts.data(), sc) == 0 && counts.back() == -7 && sc[0] == stored && sc[1] + sc[2] == stored);
            int64_t total = 0;
            for (size_t k = 0; k + 1 < counts.size(); k++) total += counts[k];
            CHECK(total == sc[1]);
        }
    return 0;
}

int main()
{
    fake_hip::set_model("k_pairs_lift", model_lift);
    fake_hip::set_model("k_pairs_emitILb0E", model_emit<false>);
    fake_hip::set_model("k_pairs_emitILb1E", model_emit<true>);
    fake_hip::set_model("k_pairs_law", model_law);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_lift_reduce", model_reduce);
    fake_hip::set_model("k_zoom_rowstart", model_zoom_rowstart);
    fake_hip::set_model("k_zoom_words", model_zoom_words);
    fake_hip::set_model("k_zoom_reduce", model_zoom_reduce);

    const Fixture fx;
    const Table tab;
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Chunk small(5, 1), mid(50, 2), big(500, 3);

    // ---- nothing without a state or a session
    CHECK(tab.begin(c) != 0 && std::strstr(ig_last_error(), "state"));
    CHECK(ig_pairs_end(c) != 0 && std::strstr(ig_last_error(), "no session"));
    CHECK(ig_pairs_clear(c) != 0 && std::strstr(ig_last_error(), "no session"));
    CHECK(small.lift(c) != 0 && std::strstr(ig_last_error(), "no session") && small.untouched());
    if (fx.fresh(c)) return 1;
    {
        int64_t U = -7, E = -7, sc[8] = {-7};
        CHECK(ig_pairs_pixels_build(c, 0, 0, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "no session") && U == -7 && E == -7 && sc[0] == -7);
    }

    // ---- the refusals of the table: on the host, before any device work
    {
        const long before = fake_hip::allocations();
        Table t = tab;
        t.rowptr[1] = 4, t.rowptr[2] = 3;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "decreases"));
        t = tab, t.rowptr[3] = 4;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "src_rowptr"));
        t = tab, t.start[1] = 9;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "overlap"));
        t = tab, t.end[4] = 6;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "interval 4 is"));
        t = tab, t.scaffold[0] = 2;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "scaffold 2 of 2"));
        t = tab, t.position[2] = 4;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "position"));
        t = tab, t.new_start[2] = 15;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "beyond its scaffold"));
        t = tab, t.len[0] = (int64_t)1 << 31;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "2^31 - 1"));
        t = tab, t.bin_unit[3] = 4;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "bin unit"));
        t = tab, t.reserve = -1;
        CHECK(t.begin(c) != 0 && std::strstr(ig_last_error(), "bad sizes"));
        CHECK(ig_pairs_begin(c, nullptr, 3, tab.start.data(), tab.end.data(), tab.new_start.data(), tab.scaffold.data(), tab.reversed.data(), tab.position.data(), 5,
                             tab.len.data(), 2, tab.bin_unit.data(), 4, 4, 0) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_pairs_begin(c, tab.rowptr.data(), 3, tab.start.data(), tab.end.data(), tab.new_start.data(), tab.scaffold.data(), tab.reversed.data(), tab.position.data(), 5,
                             tab.len.data(), (1 << 30) + 1, tab.bin_unit.data(), 4, 4, 0) != 0 && std::strstr(ig_last_error(), "2^30")); // (refused before the lengths are read)
        CHECK(fake_hip::allocations() == before); // none of them reached the device
        CHECK(ig_set_shard(c, 0, 2) == 0 && tab.begin(c) != 0 && std::strstr(ig_last_error(), "one handle") && ig_set_shard(c, 0, 1) == 0);
        CHECK(ig_pairs_end(c) != 0); // none of them left a session
    }

    // ---- begin twice; the store grows across the chunks (reserve: 1 pair); pixels, a coarsening and the law behind every chunk
    CHECK(tab.begin(c) == 0);
    CHECK(tab.begin(c) != 0 && std::strstr(ig_last_error(), "a session is open"));
    int64_t stored = 0;
    {
        int64_t U, E, sc[8];
        CHECK(ig_pairs_pixels_build(c, 1, 0, &U, &E, sc) == 0 && U == 4 && E == 0 && sc[0] == 0); // an empty store: empty rows
        CHECK(law(c, 0) == 0);
    }
    for (Chunk* ch : {&small, &mid, &big, &small}) {
        CHECK(ch->lift(c) == 0 && ch->consistent() && ch->sc[5] == stored + ch->sc[1]);
        stored = ch->sc[5];
        CHECK(all_pixels(c, stored) == 0 && law(c, stored) == 0);
    }
    CHECK(stored > 20 && stored < 560); // (some pairs of every status: the store has grown from its one reserved pair several times)
    CHECK(big.lift(c, false) == 0 && big.sc[5] == stored + big.sc[1] && big.s1[0] == -7); // no per-pair outputs: nothing of them written
    stored = big.sc[5];
    {   // some of the nine outputs only, a negative count: refused, the store as it was
        int64_t sc[8] = {-7};
        CHECK(ig_pairs_lift(c, small.c1.data(), small.p1.data(), small.c2.data(), small.p2.data(), nullptr, 5, small.s1.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, sc) != 0 && std::strstr(ig_last_error(), "together") && sc[0] == -7);
        CHECK(ig_pairs_lift(c, small.c1.data(), small.p1.data(), small.c2.data(), small.p2.data(), nullptr, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, sc) != 0 && sc[0] == -7);
        CHECK(ig_pairs_lift(c, nullptr, small.p1.data(), small.c2.data(), small.p2.data(), nullptr, 5, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, sc) != 0 && sc[0] == -7);
        CHECK(ig_pairs_lift(c, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sc) == 0 &&
              sc[0] == 0 && sc[5] == stored); // an empty chunk
        CHECK(all_pixels(c, stored) == 0);
    }

    // ---- the refusals of the pixels and of the law: each leaves nothing to fetch, the store as it was
    {
        int64_t U = -7, E = -7, sc[8] = {-7};
        CHECK(all_pixels(c, stored) == 0);
        CHECK(ig_pairs_pixels_build(c, 7, 0, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "kind") && U == -7 && sc[0] == -7 && nothing_built(c));
        CHECK(ig_pairs_pixels_build(c, 2, 0, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "bin size") && nothing_built(c));
        CHECK(ig_pairs_pixels_build(c, 2, (int64_t)1 << 31, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "bin size") && U == -7);
        CHECK(ig_pairs_pixels_build(c, 0, 0, nullptr, &E, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        g_no_heads = true; // the device reports no head among the entries: caught, nothing left
        CHECK(ig_pairs_pixels_build(c, 1, 0, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "distinct") && U == -7 && nothing_built(c));
        g_no_heads = false;
        g_free_bytes = 4096; // neither the rows nor a larger store fit what is free: refused with the bytes named
        CHECK(ig_pairs_pixels_build(c, 1, 0, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && U == -7 && nothing_built(c));
        Chunk huge(5000, 4);
        CHECK(huge.lift(c) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && huge.untouched());
        g_free_bytes = (size_t)1 << 34;
        g_lose_a_pair = true; // the device counts a pair less than it was given: caught, the store as it was
        CHECK(mid.lift(c) != 0 && std::strstr(ig_last_error(), "device error") && mid.sc[0] == -7);
        g_lose_a_pair = false;
        CHECK(all_pixels(c, stored) == 0 && law(c, stored) == 0);
        std::vector<int64_t> counts(4 * 511, -7), edges = {0, 5, 3};
        CHECK(ig_pairs_law(c, edges.data(), 3, 1, counts.data(), sc) != 0 && std::strstr(ig_last_error(), "ascending") && counts[0] == -7);
        CHECK(ig_pairs_law(c, edges.data(), 1, 1, counts.data(), sc) != 0 && ig_pairs_law(c, edges.data(), 513, 1, counts.data(), sc) != 0 && counts[0] == -7);
        CHECK(ig_pairs_law(c, nullptr, 2, 1, counts.data(), sc) != 0 && ig_pairs_law(c, edges.data(), 2, 1, nullptr, sc) != 0);
    }

    // ---- the timed passes: the store holds the chunk once behind them
    {
        std::vector<float> ms(2 * 9, -7.0f);
        std::vector<int64_t> edges = {0, 4, 16, 64};
        int64_t ck = -7;
        CHECK(ig_debug_pairs_time(c, big.c1.data(), big.p1.data(), big.c2.data(), big.p2.data(), big.strands.data(), 500, 2, 4, edges.data(), 4, 2, ms.data(), &ck) == 0);
        CHECK(ms[17] != -7.0f && ck != -7);
        CHECK(big.lift(c) == 0 && big.sc[5] == 2 * big.sc[1]);
        CHECK(ig_debug_pairs_time(c, big.c1.data(), big.p1.data(), big.c2.data(), big.p2.data(), nullptr, 500, 2, 4, edges.data(), 4, 0, ms.data(), &ck) != 0);
        CHECK(ig_debug_pairs_time(c, big.c1.data(), big.p1.data(), big.c2.data(), big.p2.data(), nullptr, 500, 2, 4, edges.data(), 4, 1, nullptr, &ck) != 0);
        CHECK(ig_pairs_clear(c) == 0 && big.lift(c) == 0 && big.sc[5] == big.sc[1]);
        stored = big.sc[5];
    }

    // ---- a session does not outlive its genome: a new state, every call refused, the session ended and begun again
    {
        std::vector<int32_t> soa = fx.soa;
        soa[(size_t)13 * Fixture::N + 7] = -1; // bin 7 turned round
        CHECK(ig_upload_state(c, soa.data(), Fixture::N) == 0);
        int64_t U = -7, E = -7, sc[8] = {-7};
        std::vector<int64_t> counts(4, -7), edges = {0, 100};
        CHECK(small.lift(c) != 0 && std::strstr(ig_last_error(), "the genome changed") && small.untouched());
        CHECK(ig_pairs_pixels_build(c, 1, 0, &U, &E, sc) != 0 && std::strstr(ig_last_error(), "the genome changed") && U == -7);
        CHECK(ig_pairs_law(c, edges.data(), 2, 1, counts.data(), sc) != 0 && std::strstr(ig_last_error(), "the genome changed") && counts[0] == -7);
        CHECK(ig_pairs_end(c) == 0 && ig_pairs_end(c) != 0 && tab.begin(c) == 0 && small.lift(c) == 0 && small.consistent());
        CHECK(fx.state(c) == 0 && small.lift(c) != 0 && ig_pairs_end(c) == 0);
    }

    // ---- every allocation of a session fails once: an error that names hipMalloc, nothing leaked, and the next session works
    {
        Chunk a(700, 5), b(40, 6);
        const auto session = [&]() -> int {
            (void)ig_pairs_end(c); // (whatever the turn before left open)
            int rc = tab.begin(c);
            if (!rc) rc = b.lift(c);
            if (!rc) rc = a.lift(c); // the store grows, the staging arrays too
            int64_t U, E, sc[8];
            if (!rc) rc = ig_pairs_pixels_build(c, 2, 3, &U, &E, sc);
            if (!rc) rc = law(c, a.sc[5]);
            return rc;
        };
        if (allocation_failure_sweep(fx, c, 120, 60, 40, 30, session, [&] { return true; }, [&] { return session() == 0 && all_pixels(c, a.sc[5]) == 0; })) return 1;
    }

    // ---- a failed lift in front of ig_destroy; a live session with a built snapshot in front of ig_destroy
    (void)ig_pairs_end(c);
    CHECK(tab.begin(c) == 0 && small.lift(c) == 0);
    CHECK(failed_call_before_destroy(c, 1, [&] { return big.lift(c); }) != 0);
    if (fx.fresh(c)) return 1;
    CHECK(tab.begin(c) == 0 && big.lift(c) == 0 && all_pixels(c, big.sc[5]) == 0);
    ig_destroy(c);
    std::printf("pairs harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
