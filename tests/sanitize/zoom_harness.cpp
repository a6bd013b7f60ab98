// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the fixed-resolution maps (csrc/ig_host_zoom.inc: the lift and
// the balancing's build with a caller's unit per position, the coarsening of a built level, the debug entry over caller data) with the
// sort and reduction they share with the other reports (csrc/ig_host_rows.inc): a stand-alone program on the fake HIP runtime
// (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is checked against the real allocation sizes).
// The models below script what steers the host -- the keys, the entries per row, the segments' starts, the words, the work lists of
// the three sort forms, the heads -- with protocol-conforming values; the sums mean nothing here, memory safety, the sizes of the
// buffers, the lifetime of the snapshot through build / coarsen / release and every refusal are the subject.  Built and run by
// tests/test_zoom_levels_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
enum { SC_IN = 0, SC_KEPT = 1, SC_CKEPT = 2, BAL_NS_KEPT = 3, BAL_NS_ENTRIES = 4 };

static long long g_entries = 0; // entries the emit models make
static bool g_no_heads = false; // the reduction finds no head: a device error the host must catch

static size_t g_free_bytes = (size_t)1 << 34; // what the device reports free
// the fake runtime has no hipMemGetInfo (the library refers to it weakly): this program brings its own, so the check runs here
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static u64 row_of_entry(long long e, int U) { return (u64)((e * 2654435761ll) % (long long)std::max(U - 2, 1)); }

static void model_heads(void** a, dim3, dim3)
{
    const int T = *(int*)a[2];
    u64* head = *(u64**)a[3];
    for (int r = 0; r < T; r++) head[r] = r % 2 == 0;
}
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
static void model_lift_keys(void** a, dim3, dim3)
{
    const int* pix = *(const int**)a[0];
    const int M = *(int*)a[1], T = *(int*)a[2];
    const u64* incl = *(const u64**)a[3];
    int* key = *(int**)a[4];
    for (int s = 0; s < M; s++) key[s] = pix[s] + (incl && T > 0 ? (int)(incl[T - 1] & 0) : 0);
}
static void model_zoom_keys(void** a, dim3, dim3) // k_zoom_keys: reads the pixel of every sub-fragment and the whole table, writes every key
{
    const int* pix = *(const int**)a[0];
    const int M = *(int*)a[1], T = *(int*)a[2];
    const int* unit = *(const int**)a[3];
    int* key = *(int**)a[4];
    int last = 0;
    for (int r = 0; r < T; r++) last = unit[r];
    for (int s = 0; s < M; s++) key[s] = pix[s] >= 0 && pix[s] < T ? unit[pix[s]] : -1 + (last & 0);
}
static void model_lift_count(void** a, dim3, dim3) // k_lift_pass<false, *>
{
    const int* key = *(const int**)a[3];
    const int U = *(int*)a[4];
    u64 *counter = *(u64**)a[5], *sc = *(u64**)a[8];
    (void)key[0];
    for (long long e = 0; e < g_entries; e++) counter[row_of_entry(e, U)]++;
    sc[SC_IN] += (u64)g_entries, sc[SC_KEPT] += (u64)g_entries, sc[SC_CKEPT] += (u64)g_entries;
}
static void model_lift_scatter(void** a, dim3, dim3) // k_lift_pass<true, *>
{
    const int U = *(int*)a[4];
    u64 *cursor = *(u64**)a[5], *ent = *(u64**)a[6];
    const u64 n_ent = *(u64*)a[7];
    for (long long e = 0; e < g_entries; e++) {
        const u64 row = row_of_entry(e, U), slot = cursor[row]++;
        if (slot < n_ent) ent[slot] = ((u64)(e % std::max(U, 1)) << 32) | 1ull;
    }
}
static void model_bal_count(void** a, dim3, dim3)
{
    const int U = *(int*)a[4];
    u64 *counter = *(u64**)a[6], *total = *(u64**)a[7], *sc = *(u64**)a[10];
    const long long n = g_entries & ~1ll;
    for (long long e = 0; e < n; e++) counter[row_of_entry(e, U)]++, total[row_of_entry(e, U)] += 1;
    sc[BAL_NS_ENTRIES] += (u64)n;
    sc[BAL_NS_KEPT] += (u64)n / 2;
}
static void model_bal_scatter(void** a, dim3, dim3)
{
    const int U = *(int*)a[4];
    u64 *cursor = *(u64**)a[6], *ent = *(u64**)a[8];
    const u64 n_ent = *(u64*)a[9];
    for (long long e = 0; e < (g_entries & ~1ll); e++) {
        const u64 row = row_of_entry(e, U), slot = cursor[row]++;
        if (slot < n_ent) ent[slot] = ((u64)(e % std::max(U, 1)) << 32) | 1ull;
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
// the coarsening's three kernels, as the device runs them: every word they read and write is the real one
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
        out_cnt[e] += fine_cnt[segstart[R] + (word[e] & 0xffffffffull)]; // (an index beyond the segment: a heap overflow the sanitizer reports)
        row_heads[R]++;
    }
}

struct Level {
    int64_t U = 0, E = 0, sc[8];
    std::vector<int64_t> rowptr, count;
    std::vector<int32_t> col;
};

static int fetch_all(ig_ctx* c, Level& v)
{
    v.rowptr.assign((size_t)v.U + 1, -7), v.col.assign((size_t)v.E + 1, -7), v.count.assign((size_t)v.E + 1, -7);
    CHECK(ig_assembly_contacts_rows(c, v.rowptr.data(), v.U + 1) == 0 && v.rowptr[0] == 0 && v.rowptr[(size_t)v.U] == v.E);
    CHECK(ig_assembly_contacts_rows(c, v.rowptr.data(), v.U) != 0);
    CHECK(ig_assembly_contacts_fetch(c, 0, v.E, v.col.data(), v.count.data()) == 0 && v.col[(size_t)v.E] == -7 && v.count[(size_t)v.E] == -7);
    CHECK(ig_assembly_contacts_fetch(c, 1, v.E, v.col.data(), v.count.data()) != 0);
    for (int64_t e = 0; e < v.E; e++) CHECK(v.col[(size_t)e] >= 0 && v.col[(size_t)e] < v.U && v.count[(size_t)e] >= 1);
    return 0;
}
static int build_units(ig_ctx* c, const std::vector<int32_t>& unit, int64_t n_units, Level& v)
{
    for (int k = 0; k < 8; k++) v.sc[k] = -7;
    v.E = -7;
    v.U = n_units;
    return ig_assembly_contacts_build_units(c, unit.data(), (int64_t)unit.size(), n_units, &v.E, v.sc);
}
static int coarsen(ig_ctx* c, const std::vector<int32_t>& map, int64_t n_units, int64_t n_coarse, Level& v)
{
    for (int k = 0; k < 8; k++) v.sc[k] = -7;
    v.E = -7;
    v.U = n_coarse;
    return ig_assembly_contacts_coarsen(c, map.data(), n_units, n_coarse, &v.E, v.sc);
}
static bool untouched(const Level& v) { return v.E == -7 && v.sc[0] == -7 && v.sc[7] == -7; }
static bool nothing_built(ig_ctx* c)
{
    int32_t col = -7;
    int64_t cnt = -7, rows[2] = {-7, -7};
    return ig_assembly_contacts_fetch(c, 0, 0, &col, &cnt) != 0 && std::strstr(ig_last_error(), "nothing is built") && ig_assembly_contacts_rows(c, rows, 2) != 0 &&
           col == -7 && rows[0] == -7;
}
static std::vector<int32_t> thirds(int64_t U)
{
    std::vector<int32_t> m((size_t)U);
    for (int64_t u = 0; u < U; u++) m[(size_t)u] = (int32_t)(u / 3);
    return m;
}

int main()
{
    fake_hip::set_model("k_lift_heads", model_heads);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_lift_keys", model_lift_keys);
    fake_hip::set_model("k_zoom_keys", model_zoom_keys);
    fake_hip::set_model("k_lift_passILb0E", model_lift_count);
    fake_hip::set_model("k_lift_passILb1E", model_lift_scatter);
    fake_hip::set_model("k_bal_emitILb0E", model_bal_count);
    fake_hip::set_model("k_bal_emitILb1E", model_bal_scatter);
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
    const int M = Fixture::M;
    const int64_t Z = fx.Z;
    // the caller's table: two positions to a unit, every other unit without a position
    const int64_t U = M;
    std::vector<int32_t> unit((size_t)M);
    for (int r = 0; r < M; r++) unit[(size_t)r] = r / 2 * 2;

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Level v, w;
    g_entries = 50;
    if (bring_up_ladder(fx, c, [&](bool) { return build_units(c, unit, U, v); }, [&] { return untouched(v); }, true, PARAMS_NEVER)) return 1;

    // ---- the refusals of the build: on the host, before any device work; the outputs untouched, nothing built, the next build works
    {
        CHECK(build_units(c, unit, U, v) == 0 && fetch_all(c, v) == 0);
        const long before = fake_hip::allocations();
        std::vector<int32_t> bad = unit;
        std::swap(bad[5], bad[6]);
        CHECK(build_units(c, bad, U, v) != 0 && std::strstr(ig_last_error(), "not monotone") && untouched(v) && nothing_built(c));
        bad = unit, bad[(size_t)M - 1] = (int32_t)U;
        CHECK(build_units(c, bad, U, v) != 0 && std::strstr(ig_last_error(), "out of range") && untouched(v) && nothing_built(c));
        bad = unit, bad[0] = -1;
        CHECK(build_units(c, bad, U, v) != 0 && std::strstr(ig_last_error(), "out of range") && untouched(v));
        CHECK(build_units(c, unit, (int64_t)1 << 31, v) != 0 && std::strstr(ig_last_error(), "2^31") && untouched(v));
        CHECK(build_units(c, unit, -1, v) != 0 && untouched(v));
        CHECK(ig_assembly_contacts_build_units(c, nullptr, M, U, &v.E, v.sc) != 0 && std::strstr(ig_last_error(), "NULL") && untouched(v));
        CHECK(ig_assembly_contacts_build_units(c, unit.data(), M, U, nullptr, v.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(fake_hip::allocations() == before); // none of them reached the device
        bad.assign(unit.begin(), unit.end() - 1);
        CHECK(build_units(c, bad, U, v) != 0 && std::strstr(ig_last_error(), "positions") && untouched(v) && nothing_built(c));
        CHECK(build_units(c, unit, U, v) == 0 && v.sc[5] == M && v.sc[6] == U && v.sc[7] == v.E);
    }

    // ---- no entry, a few (segments of the short form), many (lds and long segments under lowered limits): the build, a coarsening, a
    // coarsening behind it, down to one unit
    for (long long entries : {0ll, 50ll, (long long)Z}) {
        g_entries = entries;
        for (int limits = 0; limits < 3; limits++) {
            CHECK(ig_debug_assembly_contacts_limits(c, limits == 0 ? 0 : limits == 1 ? 2 : 1, limits == 0 ? 0 : limits == 1 ? 4 : 1) == 0);
            for (int combine = 0; combine < 2; combine++) {
                CHECK(ig_debug_assembly_contacts_combine(c, combine) == 0);
                CHECK(build_units(c, unit, U, v) == 0 && v.E == entries && v.sc[SC_KEPT] == entries && v.sc[6] == U && fetch_all(c, v) == 0);
            }
            const int64_t C1 = (U + 2) / 3, C2 = (C1 + 2) / 3;
            CHECK(coarsen(c, thirds(U), U, C1, w) == 0 && w.E == entries && w.sc[0] == entries && w.sc[1] == entries && w.sc[2] == v.sc[2] && w.sc[5] == M && w.sc[6] == C1);
            CHECK(fetch_all(c, w) == 0);
            int64_t forms[8];
            CHECK(ig_debug_assembly_contacts_forms(c, forms) == 0 && forms[1] + forms[3] + forms[5] <= entries);
            CHECK(coarsen(c, thirds(C1), C1, C2, w) == 0 && w.E == entries && w.sc[6] == C2 && fetch_all(c, w) == 0);
            CHECK(coarsen(c, std::vector<int32_t>((size_t)C2, 0), C2, 1, w) == 0 && w.sc[6] == 1 && fetch_all(c, w) == 0 && w.rowptr[1] == entries);
            CHECK(coarsen(c, std::vector<int32_t>(1, 4), 1, 9, w) == 0 && w.sc[6] == 9 && fetch_all(c, w) == 0); // coarse units no unit maps to
            // a level 1 snapshot is coarsened as well
            int64_t nu = 0;
            CHECK(ig_assembly_contacts_build(c, 1, &nu, &v.E, v.sc) == 0 && nu == M / 2);
            CHECK(coarsen(c, thirds(nu), nu, (nu + 2) / 3, w) == 0 && w.E == entries && fetch_all(c, w) == 0);
        }
    }
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && ig_debug_assembly_contacts_combine(c, 1) == 0);

    // ---- the refusals of the coarsening: each leaves nothing to fetch
    g_entries = 300;
    {
        const int64_t C1 = (U + 2) / 3;
        const std::vector<int32_t> m = thirds(U);
        CHECK(ig_assembly_contacts_release(c) == 0);
        CHECK(coarsen(c, m, U, C1, w) != 0 && std::strstr(ig_last_error(), "nothing is built") && untouched(w));
        int64_t nu = 0;
        CHECK(ig_assembly_contacts_build(c, 0, &nu, &v.E, v.sc) == 0 && nu == M);
        CHECK(coarsen(c, thirds(M), M, (M + 2) / 3, w) != 0 && std::strstr(ig_last_error(), "level 0") && untouched(w) && nothing_built(c));
        CHECK(build_units(c, unit, U, v) == 0);
        CHECK(coarsen(c, m, U - 1, C1, w) != 0 && std::strstr(ig_last_error(), "units") && untouched(w) && nothing_built(c));
        std::vector<int32_t> bad = m;
        std::swap(bad[2], bad[3]);
        CHECK(build_units(c, unit, U, v) == 0);
        CHECK(coarsen(c, bad, U, C1, w) != 0 && std::strstr(ig_last_error(), "not monotone") && untouched(w) && nothing_built(c));
        bad = m, bad[(size_t)U - 1] = (int32_t)C1;
        CHECK(build_units(c, unit, U, v) == 0);
        CHECK(coarsen(c, bad, U, C1, w) != 0 && std::strstr(ig_last_error(), "out of range") && untouched(w) && nothing_built(c));
        CHECK(build_units(c, unit, U, v) == 0);
        CHECK(coarsen(c, m, U, (int64_t)1 << 31, w) != 0 && std::strstr(ig_last_error(), "2^31") && untouched(w) && nothing_built(c));
        CHECK(build_units(c, unit, U, v) == 0);
        CHECK(ig_assembly_contacts_coarsen(c, nullptr, U, C1, &w.E, w.sc) != 0 && std::strstr(ig_last_error(), "NULL") && nothing_built(c));
        // the device reports no head among the words: caught, nothing left
        CHECK(build_units(c, unit, U, v) == 0);
        g_no_heads = true;
        CHECK(coarsen(c, m, U, C1, w) != 0 && std::strstr(ig_last_error(), "distinct") && untouched(w) && nothing_built(c));
        g_no_heads = false;
        // the temporaries do not fit what is free: refused with the bytes named, before anything is allocated by their number
        CHECK(build_units(c, unit, U, v) == 0);
        g_free_bytes = 4096;
        const long before = fake_hip::allocations();
        CHECK(coarsen(c, m, U, C1, w) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && untouched(w) && nothing_built(c));
        CHECK(fake_hip::allocations() - before < 4);
        g_free_bytes = (size_t)1 << 34;
        CHECK(build_units(c, unit, U, v) == 0 && coarsen(c, m, U, C1, w) == 0 && fetch_all(c, w) == 0); // and the next ones work
    }

    // ---- the balancing's build with the same table
    {
        int64_t E = -7, sc[8];
        for (int k = 0; k < 8; k++) sc[k] = -7;
        std::vector<int32_t> bad = unit;
        std::swap(bad[5], bad[6]);
        CHECK(ig_balance_build_units(c, bad.data(), M, U, 2, &E, sc) != 0 && std::strstr(ig_last_error(), "not monotone") && E == -7 && sc[0] == -7);
        CHECK(ig_balance_build_units(c, unit.data(), M - 1, U, 2, &E, sc) != 0 && std::strstr(ig_last_error(), "positions") && E == -7);
        CHECK(ig_balance_build_units(c, unit.data(), M, U, 0, &E, sc) != 0 && std::strstr(ig_last_error(), "ignore_diags") && E == -7);
        CHECK(ig_balance_fetch(c, 0, 0, nullptr, nullptr) != 0);
        CHECK(ig_balance_build_units(c, unit.data(), M, U, 2, &E, sc) == 0 && E == 300 && sc[5] == M && sc[6] == U && sc[7] == E);
        std::vector<int64_t> rowptr((size_t)U + 1), nnz((size_t)U), total((size_t)U);
        CHECK(ig_balance_rows(c, rowptr.data(), nnz.data(), total.data(), U + 1) == 0 && rowptr[(size_t)U] == E);
        std::vector<double> b0((size_t)U, 1.0), bb((size_t)U), marg((size_t)U), var(3);
        int32_t n_it = -7, conv = -7;
        CHECK(ig_balance_run(c, b0.data(), 0.0, 3, bb.data(), marg.data(), var.data(), &n_it, &conv) == 0);
        int64_t nu = 0;
        CHECK(ig_balance_build(c, 1, 2048, 2, &nu, &E, sc) == 0 && nu == M / 2); // the three levels behave as before
        CHECK(ig_balance_release(c) == 0);
        CHECK(fetch_all(c, w) == 0); // (the lift's snapshot is its own)
    }

    // ---- the coarsening over caller data: a RowBuf of its own, the result on the host
    {
        const int64_t rowptr[6] = {0, 2, 2, 5, 5, 6}, count[6] = {1, (int64_t)1 << 40, 3, 4, (int64_t)1 << 41, 6};
        const int32_t col[6] = {0, 3, 2, 3, 4, 4}, map[5] = {0, 0, 2, 2, 3};
        int64_t n_out = -7, forms[8], out_rowptr[6];
        int32_t out_col[6];
        int64_t out_count[6];
        CHECK(ig_debug_zoom_fetch(c, out_rowptr, 6, out_col, out_count, 6) != 0 && std::strstr(ig_last_error(), "nothing is built"));
        CHECK(ig_debug_zoom_coarsen(c, rowptr, col, count, 5, map, 5, &n_out, forms) == 0 && n_out == 6);
        CHECK(ig_debug_zoom_fetch(c, out_rowptr, 5, out_col, out_count, 6) != 0 && ig_debug_zoom_fetch(c, out_rowptr, 6, out_col, out_count, 5) != 0);
        CHECK(ig_debug_zoom_fetch(c, out_rowptr, 6, out_col, out_count, 6) == 0 && out_rowptr[0] == 0 && out_rowptr[1] == 2 && out_rowptr[2] == 2 && out_rowptr[5] == 6);
        const int32_t down[5] = {0, 1, 0, 2, 3}, far[5] = {0, 0, 2, 2, 5}, wide[6] = {0, 3, 2, 3, 5, 4};
        const int64_t back[6] = {0, 2, 1, 5, 5, 6};
        CHECK(ig_debug_zoom_coarsen(c, rowptr, col, count, 5, down, 5, &n_out, forms) != 0 && std::strstr(ig_last_error(), "not monotone"));
        CHECK(ig_debug_zoom_fetch(c, out_rowptr, 6, out_col, out_count, 6) != 0); // a failed call leaves nothing to fetch
        CHECK(ig_debug_zoom_coarsen(c, rowptr, col, count, 5, far, 5, &n_out, forms) != 0 && std::strstr(ig_last_error(), "out of range"));
        CHECK(ig_debug_zoom_coarsen(c, rowptr, wide, count, 5, map, 5, &n_out, forms) != 0 && std::strstr(ig_last_error(), "column"));
        CHECK(ig_debug_zoom_coarsen(c, back, col, count, 5, map, 5, &n_out, forms) != 0 && std::strstr(ig_last_error(), "decreases"));
        CHECK(ig_debug_zoom_coarsen(c, rowptr, col, count, 5, map, 5, nullptr, forms) != 0 && std::strstr(ig_last_error(), "NULL"));
        const int64_t none[1] = {0};
        CHECK(ig_debug_zoom_coarsen(c, none, nullptr, nullptr, 0, nullptr, 0, &n_out, forms) == 0 && n_out == 0);
        CHECK(ig_debug_zoom_coarsen(c, none, nullptr, nullptr, 0, nullptr, 3, &n_out, forms) == 0 && n_out == 0 && ig_debug_zoom_fetch(c, out_rowptr, 4, nullptr, nullptr, 0) == 0);
        for (int n = 0; n < 24; n++) { // every allocation of the call fails once: nothing to fetch (and nothing leaked: LeakSanitizer looks at the exit)
            fake_hip::fail_allocation_in(n);
            const int rc = ig_debug_zoom_coarsen(c, rowptr, col, count, 5, map, 5, &n_out, forms);
            fake_hip::fail_allocation_in(-1);
            if (rc) CHECK(std::strstr(ig_last_error(), "hipMalloc") && ig_debug_zoom_fetch(c, out_rowptr, 6, out_col, out_count, 6) != 0);
        }
    }

    // ---- every allocation of a build and of a coarsening behind it fails once: an error, nothing leaked, nothing built, the next works
    {
        const int64_t C1 = (U + 2) / 3;
        const std::vector<int32_t> m = thirds(U);
        CHECK(ig_debug_assembly_contacts_limits(c, 2, 4) == 0); // (long segments: the scratch buffer and the runs' items are allocated too)
        const auto both = [&] {
            int rc = build_units(c, unit, U, v);
            if (!rc) rc = coarsen(c, m, U, C1, w);
            return rc;
        };
        if (allocation_failure_sweep(fx, c, 60, 30, 20, 20, both, [&] { return nothing_built(c); },
                                     [&] { return ig_debug_assembly_contacts_limits(c, 2, 4) == 0 && both() == 0 && fetch_all(c, w) == 0; }))
            return 1;
    }

    // ---- the timed coarsening: the snapshot survives
    {
        std::vector<float> ms(2 * 6, -7.0f);
        int64_t ck = -7, ck2 = -7;
        CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && build_units(c, unit, U, v) == 0 && fetch_all(c, v) == 0);
        const std::vector<int32_t> m = thirds(U);
        CHECK(ig_debug_zoom_time(c, m.data(), U, (U + 2) / 3, 2, ms.data(), &ck) == 0 && ms[11] != -7.0f);
        CHECK(ig_debug_zoom_time(c, nullptr, 0, 0, 1, ms.data(), &ck2) == 0 && ig_debug_zoom_time(c, nullptr, 0, 0, 1, ms.data(), nullptr) == 0);
        Level again = v;
        CHECK(fetch_all(c, again) == 0 && again.col == v.col && again.count == v.count && again.rowptr == v.rowptr);
        CHECK(ig_debug_zoom_time(c, m.data(), U - 1, (U + 2) / 3, 1, ms.data(), &ck) != 0 && ig_debug_zoom_time(c, m.data(), U, (U + 2) / 3, 0, ms.data(), &ck) != 0);
        CHECK(ig_debug_zoom_time(c, m.data(), U, (U + 2) / 3, 1, nullptr, &ck) != 0 && fetch_all(c, again) == 0);
        CHECK(ig_assembly_contacts_release(c) == 0 && ig_debug_zoom_time(c, nullptr, 0, 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "nothing to coarsen"));
    }

    // ---- release with a snapshot resident; a new upload of the contacts releases it; ig_destroy behind a failed coarsening and with one resident
    CHECK(build_units(c, unit, U, v) == 0 && ig_assembly_contacts_release(c) == 0 && nothing_built(c) && ig_assembly_contacts_release(c) == 0);
    CHECK(build_units(c, unit, U, v) == 0 && coarsen(c, thirds(U), U, (U + 2) / 3, w) == 0 && fx.contacts(c) == 0 && nothing_built(c));
    CHECK(build_units(c, unit, U, v) == 0);
    CHECK(failed_call_before_destroy(c, 3, [&] { return coarsen(c, thirds(U), U, (U + 2) / 3, w); }) != 0);
    if (fx.fresh(c)) return 1;
    CHECK(build_units(c, unit, U, v) == 0 && coarsen(c, thirds(U), U, (U + 2) / 3, w) == 0);
    ig_destroy(c);
    std::printf("zoom harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
