// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the pyramid's contact levels (csrc/ig_host_pyr.inc: the session,
// the upload in pieces, the two RowBufs that swap roles from level to level, the table of a remap, the degrees, the fetched stretches,
// the refusal of a sum of 2^31 or more) with the sort and reduction it shares with the reports (csrc/ig_host_rows.inc): a stand-alone
// program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is checked against
// the real allocation sizes).  The models below do what the five kernels do, load for load and word for word; every level that comes out
// is compared with a brute force over a map of pixels.  Built and run by tests/test_pyramid_levels_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_rows.cuh: device code, not included here)
struct Item {
    long long off;
    int len, pad;
};
struct Long {
    long long off, scratch, len;
};

static bool g_no_heads = false;
static bool g_lose_an_entry = false; // the emit pass counts an entry less than it was given: a device error the host must catch
static size_t g_free_bytes = (size_t)1 << 34;
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static int row_of(const u64* rowptr, int U, long long e)
{
    int lo = 0, hi = U;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rowptr[mid] <= (u64)e) lo = mid;
        else hi = mid;
    }
    return lo;
}
static void model_canon(void** a, dim3, dim3)
{
    const int *x = *(const int**)a[0], *y = *(const int**)a[1];
    const long long n = *(long long*)a[2];
    u64* sc = *(u64**)a[3];
    for (long long k = 0; k < n; k++) {
        bool bad = x[k] > y[k];
        if (k > 0) bad = bad || x[k - 1] > x[k] || (x[k - 1] == x[k] && y[k - 1] >= y[k]);
        if (bad) sc[0]++;
    }
}
template <bool SCATTER, bool RAW>
static void model_emit(void** a, dim3, dim3)
{
    const int *fa = *(const int**)a[0], *fb = *(const int**)a[1], *cnt = *(const int**)a[2];
    const u64* rowptr = *(const u64**)a[3];
    const int* col = *(const int**)a[4];
    const u64* sum = *(const u64**)a[5];
    const long long n = *(long long*)a[6];
    const int U_old = *(int*)a[7];
    const int* lut = *(const int**)a[8];
    const int U_new = *(int*)a[9];
    const long long skip = *(long long*)a[10];
    u64 *counter = *(u64**)a[11], *ent = *(u64**)a[12];
    const u64 n_ent = *(u64*)a[13];
    u64* sc = *(u64**)a[14];
    for (long long k = 0; k < n - (g_lose_an_entry ? 1 : 0); k++) {
        if (!SCATTER) sc[0]++;
        if (k < skip) {
            if (!SCATTER) sc[1]++;
            continue;
        }
        int x, y, v;
        if (RAW) x = fa[k], y = fb[k], v = cnt[k];
        else x = row_of(rowptr, U_old, k), y = col[k], v = (int)sum[k];
        const bool inside = x >= 0 && y >= 0 && x < U_old && y < U_old;
        if (inside && lut) x = lut[x], y = lut[y];
        if (!inside || x < 0 || y < 0 || x >= U_new || y >= U_new) {
            if (!SCATTER) sc[2]++;
            continue;
        }
        const u64 slot = counter[std::min(x, y)]++;
        if (!SCATTER) sc[3]++;
        else if (slot < n_ent) ent[slot] = ((u64)(unsigned)std::max(x, y) << 32) | (u64)(unsigned)v;
    }
}
static void model_largest(void** a, dim3, dim3)
{
    const u64* sum = *(const u64**)a[0];
    const long long n = *(long long*)a[1];
    u64 *largest = *(u64**)a[2], *first_bad = *(u64**)a[3];
    for (long long k = 0; k < n; k++) {
        *largest = std::max(*largest, sum[k]);
        if (sum[k] >= 0x80000000ull) *first_bad = std::min(*first_bad, (u64)k);
    }
}
static void model_degrees(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int U = *(int*)a[1];
    const int* col = *(const int**)a[2];
    const u64* sum = *(const u64**)a[3];
    const long long n = *(long long*)a[4];
    unsigned* deg = *(unsigned**)a[5];
    for (long long k = 0; k < n; k++) {
        if (!sum[k]) continue;
        const int r = row_of(rowptr, U, k);
        deg[r]++;
        if (col[k] != r) deg[col[k]]++;
    }
}
static void model_expand(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int U = *(int*)a[1];
    const int* col = *(const int**)a[2];
    const u64* sum = *(const u64**)a[3];
    const long long first = *(long long*)a[4], n = *(long long*)a[5];
    int *out_row = *(int**)a[6], *out_col = *(int**)a[7], *out_cnt = *(int**)a[8];
    for (long long k = 0; k < n; k++) out_row[k] = row_of(rowptr, U, first + k), out_col[k] = col[first + k], out_cnt[k] = (int)sum[first + k];
}
// the row builder's kernels, as tests/sanitize/pre_harness.cpp models them
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

// ---- the rule by brute force: a level is a map of pixels, whose order is the level's
typedef std::map<std::pair<int, int>, long long> Pixels;
struct List {
    std::vector<int32_t> a, b;
    std::vector<int64_t> cnt;
    int U;
    List(int n, int n_frags, unsigned seed) : a((size_t)n), b((size_t)n), cnt((size_t)n), U(n_frags)
    {
        unsigned x = 99u + seed;
        auto next = [&] { return (x = x * 1664525u + 1013904223u) >> 8; };
        for (int k = 0; k < n; k++) {
            a[(size_t)k] = (int32_t)(next() % (unsigned)U);
            b[(size_t)k] = next() % 5 == 0 ? a[(size_t)k] : next() % 4 == 0 && k > 0 ? a[(size_t)k - 1] : (int32_t)(next() % (unsigned)U);
            cnt[(size_t)k] = next() % 6 == 0 ? 0 : (int64_t)(next() % 90);
        }
    }
    int begin(ig_ctx* c, int32_t* flag) const { return ig_pyr_begin(c, U, a.data(), b.data(), cnt.data(), (int64_t)a.size(), flag); }
    Pixels level() const
    {
        Pixels m;
        for (size_t k = 0; k < a.size(); k++) m[{std::min(a[k], b[k]), std::max(a[k], b[k])}] += cnt[k];
        return m;
    }
    // the remap of the list itself: entry 0 in FILE order is the one that is lost
    Pixels remap(const std::vector<int32_t>& lut, bool skip) const
    {
        Pixels m;
        for (size_t k = skip ? 1 : 0; k < a.size(); k++) {
            const int x = lut[(size_t)a[k]], y = lut[(size_t)b[k]];
            if (x >= 0 && y >= 0) m[{std::min(x, y), std::max(x, y)}] += cnt[k];
        }
        return m;
    }
};
static Pixels remap_level(const Pixels& from, const std::vector<int32_t>& lut, bool skip, int64_t* dropped)
{
    Pixels m;
    bool first = true;
    *dropped = 0;
    for (const auto& px : from) {
        if (first && skip) {
            first = false;
            continue;
        }
        first = false;
        const int x = lut[(size_t)px.first.first], y = lut[(size_t)px.first.second];
        if (x >= 0 && y >= 0) m[{std::min(x, y), std::max(x, y)}] += px.second;
        else ++*dropped;
    }
    return m;
}
// the current level of the session is `want` over U fragments: the rows, the three int32 rows in pieces, the degrees
static int level_agrees(ig_ctx* c, const Pixels& want, int U)
{
    const int64_t E = (int64_t)want.size();
    std::vector<int64_t> rowptr((size_t)U + 2, -7);
    std::vector<int32_t> row((size_t)E + 1, -7), col((size_t)E + 1, -7), cnt((size_t)E + 1, -7), deg((size_t)U + 1, -7);
    CHECK(ig_pyr_rows(c, rowptr.data(), U) != 0 && rowptr[0] == -7);
    CHECK(ig_pyr_rows(c, rowptr.data(), U + 1) == 0 && rowptr[0] == 0 && rowptr[(size_t)U] == E && rowptr[(size_t)U + 1] == -7);
    for (int64_t a = 0; a < E; a += 7) CHECK(ig_pyr_fetch(c, a, std::min<int64_t>(7, E - a), row.data() + a, col.data() + a, cnt.data() + a) == 0);
    CHECK(row[(size_t)E] == -7 && cnt[(size_t)E] == -7 && ig_pyr_fetch(c, E, 1, row.data(), col.data(), cnt.data()) != 0 && ig_pyr_fetch(c, -1, 1, row.data(), col.data(), cnt.data()) != 0);
    CHECK(ig_pyr_fetch(c, 0, 0, nullptr, nullptr, nullptr) == 0 && (E == 0 || (ig_pyr_fetch(c, 0, 1, nullptr, col.data(), cnt.data()) != 0 && std::strstr(ig_last_error(), "NULL"))));
    std::vector<int32_t> want_deg((size_t)U, 0);
    int64_t e = 0;
    for (const auto& px : want) {
        CHECK(row[(size_t)e] == px.first.first && col[(size_t)e] == px.first.second && cnt[(size_t)e] == px.second);
        CHECK(rowptr[(size_t)px.first.first] <= e && e < rowptr[(size_t)px.first.first + 1]);
        if (px.second) {
            want_deg[(size_t)px.first.first]++;
            if (px.first.first != px.first.second) want_deg[(size_t)px.first.second]++;
        }
        e++;
    }
    CHECK(ig_pyr_degrees(c, deg.data()) == 0 && deg[(size_t)U] == -7);
    for (int u = 0; u < U; u++) CHECK(deg[(size_t)u] == want_deg[(size_t)u]);
    CHECK(U == 0 || (ig_pyr_degrees(c, nullptr) != 0 && std::strstr(ig_last_error(), "NULL")));
    return 0;
}
static std::vector<int32_t> bins(int n, int factor, int* n_new)
{
    std::vector<int32_t> lut((size_t)n);
    for (int k = 0; k < n; k++) lut[(size_t)k] = k / factor;
    *n_new = (n + factor - 1) / factor;
    return lut;
}
// three levels behind the list's own: the filter's table (fragments destroyed, no entry lost), then two binnings (the first entry lost)
static int three_levels(ig_ctx* c, const List& L, bool through_matrix)
{
    int32_t flag = -7;
    int64_t E = -7, sc[8];
    std::vector<float> ms(7, -7.0f);
    CHECK(L.begin(c, &flag) == 0 && flag == 0);
    Pixels cur = L.level();
    int U = L.U;
    std::vector<int32_t> filt((size_t)U);
    int kept = 0;
    for (int k = 0; k < U; k++) filt[(size_t)k] = (k % 11 == 3 || (k >= 20 && k < 26)) ? -1 : (k % 7 == 0 ? kept : kept++);
    kept = 1 + *std::max_element(filt.begin(), filt.end()); /* (a glued fragment at the end names the id behind the last emitted one) */
    if (through_matrix) {
        CHECK(ig_pyr_matrix(c, &E, ms.data()) == 0 && E == (int64_t)cur.size() && ms[6] != -7.0f);
        CHECK(level_agrees(c, cur, U) == 0);
        CHECK(ig_pyr_matrix(c, &E, nullptr) == 0 && E == (int64_t)cur.size()); // once more: the level is made already
    }
    int64_t dropped = 0;
    Pixels next = through_matrix ? remap_level(cur, filt, false, &dropped) : L.remap(filt, false);
    CHECK(ig_pyr_remap(c, filt.data(), U, kept, 0, &E, sc, ms.data()) == 0 && E == (int64_t)next.size() && sc[4] == E && sc[1] == 0 && sc[0] == sc[2] + sc[3]);
    CHECK(!through_matrix || (sc[0] == (int64_t)cur.size() && sc[2] == dropped));
    CHECK(level_agrees(c, next, kept) == 0);
    cur = next, U = kept;
    for (int round = 0; round < 2; round++) {
        int n_new = 0;
        const std::vector<int32_t> lut = bins(U, 3, &n_new);
        next = remap_level(cur, lut, true, &dropped);
        int64_t largest = 0;
        for (const auto& px : next) largest = std::max<int64_t>(largest, px.second);
        CHECK(ig_pyr_remap(c, lut.data(), U, n_new, 1, &E, sc, nullptr) == 0 && E == (int64_t)next.size());
        CHECK(sc[0] == (int64_t)cur.size() && sc[1] == (cur.empty() ? 0 : 1) && sc[2] == 0 && sc[3] == sc[0] - sc[1] && sc[4] == E && sc[5] == largest && sc[6] == 0 && sc[7] == 0);
        CHECK(level_agrees(c, next, n_new) == 0);
        cur = next, U = n_new;
    }
    CHECK(ig_pyr_end(c) == 0);
    return 0;
}

int main()
{
    fake_hip::set_model("k_pyr_canon", model_canon);
    fake_hip::set_model("k_pyr_emitILb0ELb0E", (model_emit<false, false>));
    fake_hip::set_model("k_pyr_emitILb0ELb1E", (model_emit<false, true>));
    fake_hip::set_model("k_pyr_emitILb1ELb0E", (model_emit<true, false>));
    fake_hip::set_model("k_pyr_emitILb1ELb1E", (model_emit<true, true>));
    fake_hip::set_model("k_pyr_largest", model_largest);
    fake_hip::set_model("k_pyr_degrees", model_degrees);
    fake_hip::set_model("k_pyr_expand", model_expand);
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
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    const List small(40, 9, 1), mid(700, 61, 2), wide(3000, 200, 3);
    int32_t flag = -7;
    int64_t E = -7, sc[8] = {-7, -7, -7, -7, -7, -7, -7, -7}, rowptr[4] = {-7};
    int32_t out = -7;
    const std::vector<int32_t> ident = {0, 1, 2, 3, 4, 5, 6, 7, 8};

    // ---- nothing without a session
    CHECK(ig_pyr_end(c) != 0 && std::strstr(ig_last_error(), "no session"));
    CHECK(ig_pyr_matrix(c, &E, nullptr) != 0 && std::strstr(ig_last_error(), "no session") && E == -7);
    CHECK(ig_pyr_degrees(c, &out) != 0 && std::strstr(ig_last_error(), "no session") && out == -7);
    CHECK(ig_pyr_remap(c, ident.data(), 9, 9, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "no session") && E == -7 && sc[0] == -7);
    CHECK(ig_pyr_rows(c, rowptr, 4) != 0 && std::strstr(ig_last_error(), "no session") && rowptr[0] == -7);
    CHECK(ig_pyr_fetch(c, 0, 1, &out, &out, &out) != 0 && std::strstr(ig_last_error(), "no session") && out == -7);

    // ---- the refusals of the list: on the host, before any device work
    {
        const long before = fake_hip::allocations();
        List t = small;
        t.a[17] = 9;
        CHECK(t.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "entry 17 is (9,") && flag == -7);
        t = small, t.b[3] = -1;
        CHECK(t.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "entry 3 is (") && std::strstr(ig_last_error(), ", -1)"));
        t = small, t.cnt[39] = -2;
        CHECK(t.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "entry 39 has the count -2"));
        t = small, t.cnt[0] = (int64_t)1 << 31;
        CHECK(t.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "entry 0 has the count 2147483648"));
        t = small, t.cnt[5] = ((int64_t)1 << 32) + 5; // (a count whose low half alone would pass)
        CHECK(t.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "entry 5 has the count 4294967301"));
        CHECK(ig_pyr_begin(c, 0, small.a.data(), small.b.data(), small.cnt.data(), 40, &flag) != 0 && std::strstr(ig_last_error(), "bad sizes"));
        CHECK(ig_pyr_begin(c, 9, small.a.data(), small.b.data(), small.cnt.data(), -1, &flag) != 0 && std::strstr(ig_last_error(), "bad sizes"));
        CHECK(ig_pyr_begin(c, 9, nullptr, small.b.data(), small.cnt.data(), 40, &flag) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_pyr_begin(c, 9, small.a.data(), small.b.data(), small.cnt.data(), 40, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
        g_free_bytes = 1024;
        CHECK(small.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
        g_free_bytes = (size_t)1 << 34;
        CHECK(fake_hip::allocations() == before && flag == -7); // none of them reached the device
        CHECK(ig_pyr_end(c) != 0);                              // none of them left a session
    }

    // ---- begin twice; nothing of a level before one is made; the refusals of a table
    CHECK(small.begin(c, &flag) == 0 && flag == 0);
    CHECK(small.begin(c, &flag) != 0 && std::strstr(ig_last_error(), "a session is open"));
    CHECK(ig_pyr_degrees(c, &out) != 0 && std::strstr(ig_last_error(), "ig_pyr_matrix first") && out == -7);
    CHECK(ig_pyr_rows(c, rowptr, 4) != 0 && std::strstr(ig_last_error(), "ig_pyr_matrix first"));
    CHECK(ig_pyr_fetch(c, 0, 1, &out, &out, &out) != 0 && std::strstr(ig_last_error(), "ig_pyr_matrix first") && out == -7);
    {
        std::vector<int32_t> t = ident;
        CHECK(ig_pyr_remap(c, t.data(), 8, 8, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "the table has 8 entries, the current level 9 fragments"));
        CHECK(ig_pyr_remap(c, t.data(), 9, 10, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "10 new fragments of 9"));
        CHECK(ig_pyr_remap(c, t.data(), 9, 9, 2, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "skip_first"));
        CHECK(ig_pyr_remap(c, nullptr, 9, 9, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_pyr_remap(c, t.data(), 9, 9, 0, nullptr, sc, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
        t[4] = 2;
        CHECK(ig_pyr_remap(c, t.data(), 9, 9, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "maps fragment 4 to 2"));
        t = ident, t[8] = 9;
        CHECK(ig_pyr_remap(c, t.data(), 9, 9, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "maps fragment 8 to 9"));
        t = ident, t[0] = -2;
        CHECK(ig_pyr_remap(c, t.data(), 9, 9, 0, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "maps fragment 0 to -2") && E == -7 && sc[0] == -7);
    }
    CHECK(ig_pyr_matrix(c, &E, nullptr) == 0 && level_agrees(c, small.level(), 9) == 0);
    CHECK(ig_pyr_end(c) == 0 && ig_pyr_end(c) != 0 && std::strstr(ig_last_error(), "no session"));

    // ---- the upload in pieces smaller than the list; the two RowBufs swapping over three levels, under the default and lowered limits
    for (const int64_t piece : {(int64_t)0, (int64_t)1, (int64_t)37, (int64_t)700}) {
        CHECK(ig_debug_pyr_piece(c, piece) == 0);
        CHECK(three_levels(c, mid, true) == 0 && three_levels(c, mid, false) == 0);
    }
    CHECK(ig_debug_pyr_piece(c, -1) != 0 && ig_debug_pyr_piece(c, 0) == 0);
    CHECK(ig_debug_assembly_contacts_limits(c, 2, 4) == 0 && three_levels(c, wide, true) == 0 && three_levels(c, wide, false) == 0);
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && three_levels(c, wide, true) == 0 && three_levels(c, small, true) == 0);
    {
        // a canonical list: the flag, and the level is the list
        const Pixels lev = mid.level();
        List canon(0, mid.U, 0);
        for (const auto& px : lev) canon.a.push_back(px.first.first), canon.b.push_back(px.first.second), canon.cnt.push_back(px.second);
        CHECK(canon.begin(c, &flag) == 0 && flag == 1 && ig_pyr_matrix(c, &E, nullptr) == 0 && E == (int64_t)lev.size() && level_agrees(c, lev, mid.U) == 0);
        // everything destroyed: a level of no fragment, and a further remap of it
        const std::vector<int32_t> none((size_t)mid.U, -1);
        CHECK(ig_pyr_remap(c, none.data(), mid.U, 0, 1, &E, sc, nullptr) == 0 && E == 0 && sc[0] == (int64_t)lev.size() && sc[1] == 1 && sc[2] == sc[0] - 1 && sc[3] == 0 && sc[5] == 0);
        CHECK(level_agrees(c, Pixels(), 0) == 0);
        CHECK(ig_pyr_remap(c, nullptr, 0, 0, 1, &E, sc, nullptr) == 0 && E == 0 && sc[0] == 0 && sc[1] == 0 && level_agrees(c, Pixels(), 0) == 0);
        CHECK(ig_pyr_end(c) == 0);
        // an empty list; a level of one fragment
        List empty(0, 4, 0), one(6, 1, 5);
        CHECK(empty.begin(c, &flag) == 0 && flag == 1 && ig_pyr_matrix(c, &E, nullptr) == 0 && E == 0 && level_agrees(c, Pixels(), 4) == 0 && ig_pyr_end(c) == 0);
        CHECK(one.begin(c, &flag) == 0 && flag == 0 && ig_pyr_matrix(c, &E, nullptr) == 0 && E == 1 && level_agrees(c, one.level(), 1) == 0 && ig_pyr_end(c) == 0);
    }

    // ---- a sum of 2^31 - 1 passes, 2^31 is refused naming the pixel, and the session stays usable
    {
        List t(0, 6, 0);
        t.a = {3, 5, 5, 3, 0}, t.b = {5, 3, 5, 5, 1}, t.cnt = {2147483637, 4, 7, 6, 1};
        CHECK(t.begin(c, &flag) == 0 && ig_pyr_matrix(c, &E, nullptr) == 0 && E == 3 && level_agrees(c, t.level(), 6) == 0);
        const std::vector<int32_t> all0(6, 0);
        CHECK(ig_pyr_remap(c, all0.data(), 6, 1, 1, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "the sum of the pixel (0, 0) is 2147483654: 2^31 or more") && E == 3);
        CHECK(level_agrees(c, t.level(), 6) == 0); // the current level is still the one before the refused remap
        const std::vector<int32_t> merge = {0, 0, 1, 1, 2, 2};
        CHECK(ig_pyr_remap(c, merge.data(), 6, 3, 0, &E, sc, nullptr) == 0 && E == 3 && sc[5] == 2147483647);
        CHECK(ig_pyr_end(c) == 0);
        t.cnt[1] = 5;
        CHECK(t.begin(c, &flag) == 0);
        CHECK(ig_pyr_matrix(c, &E, nullptr) != 0 && std::strstr(ig_last_error(), "the sum of the pixel (3, 5) is 2147483648: 2^31 or more"));
        CHECK(ig_pyr_rows(c, rowptr, 4) != 0 && std::strstr(ig_last_error(), "ig_pyr_matrix first")); // the list is still the current level
        const std::vector<int32_t> drop3 = {0, 1, 2, -1, 3, 4};
        CHECK(ig_pyr_remap(c, drop3.data(), 6, 5, 0, &E, sc, nullptr) == 0 && E == 2 && level_agrees(c, t.remap(drop3, false), 5) == 0);
        CHECK(ig_pyr_end(c) == 0);
    }

    // ---- the device errors and the free-memory guard: each leaves the current level as it was
    {
        CHECK(mid.begin(c, &flag) == 0);
        g_lose_an_entry = true;
        CHECK(ig_pyr_matrix(c, &E, nullptr) != 0 && std::strstr(ig_last_error(), "device error"));
        g_lose_an_entry = false;
        g_no_heads = true;
        CHECK(ig_pyr_matrix(c, &E, nullptr) != 0 && std::strstr(ig_last_error(), "distinct"));
        g_no_heads = false;
        g_free_bytes = 4096;
        CHECK(ig_pyr_matrix(c, &E, nullptr) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
        g_free_bytes = (size_t)1 << 34;
        CHECK(ig_pyr_matrix(c, &E, nullptr) == 0 && level_agrees(c, mid.level(), mid.U) == 0);
        int n_new = 0;
        const std::vector<int32_t> lut = bins(mid.U, 3, &n_new);
        g_no_heads = true;
        CHECK(ig_pyr_remap(c, lut.data(), mid.U, n_new, 1, &E, sc, nullptr) != 0 && std::strstr(ig_last_error(), "distinct"));
        g_no_heads = false;
        CHECK(level_agrees(c, mid.level(), mid.U) == 0);
        CHECK(ig_pyr_end(c) == 0);
    }

    // ---- every allocation of a session fails once: an error that names hipMalloc, nothing leaked, and the next session works
    {
        const auto session = [&]() -> int {
            (void)ig_pyr_end(c); // (whatever the turn before left open)
            int rc = mid.begin(c, &flag);
            if (!rc) rc = ig_pyr_matrix(c, &E, nullptr);
            int32_t deg[61];
            if (!rc) rc = ig_pyr_degrees(c, deg);
            int U = mid.U;
            for (int round = 0; round < 3 && !rc; round++) {
                int n_new = 0;
                const std::vector<int32_t> lut = bins(U, 3, &n_new);
                rc = ig_pyr_remap(c, lut.data(), U, n_new, 1, &E, sc, nullptr);
                U = n_new;
            }
            int32_t r3[3];
            if (!rc && E > 0) rc = ig_pyr_fetch(c, 0, 1, r3, r3 + 1, r3 + 2);
            return rc;
        };
        if (allocation_failure_sweep(fx, c, 160, 80, 40, 40, session, [&] { return true; }, [&] { return session() == 0 && ig_pyr_end(c) == 0 && three_levels(c, mid, true) == 0; })) return 1;
    }

    // ---- a failed remap in front of ig_destroy; a live session with two levels made in front of ig_destroy
    (void)ig_pyr_end(c);
    {
        int n_new = 0;
        const std::vector<int32_t> lut = bins(mid.U, 3, &n_new);
        CHECK(mid.begin(c, &flag) == 0 && ig_pyr_matrix(c, &E, nullptr) == 0);
        CHECK(failed_call_before_destroy(c, 1, [&] { return ig_pyr_remap(c, lut.data(), mid.U, n_new, 1, &E, sc, nullptr); }) != 0);
        CHECK(ig_create(0, &c) == 0 && mid.begin(c, &flag) == 0 && ig_pyr_matrix(c, &E, nullptr) == 0);
        CHECK(ig_pyr_remap(c, lut.data(), mid.U, n_new, 1, &E, sc, nullptr) == 0 && ig_pyr_fetch(c, 0, 1, &out, &out, &out) == 0);
        ig_destroy(c);
    }
    std::printf("pyr harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
