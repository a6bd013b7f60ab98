// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the join support (csrc/ig_host_join.inc) and of the sort and
// reduction it shares with the contacts in genome coordinates (lift_sort_rows, lift_reduce_rows in csrc/ig_host_rows.inc): a
// stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is
// checked against the real allocation sizes).  The models below script what steers the host -- the number of contigs, the entries per
// row, the work lists of the three sort forms, the heads, the largest model value -- with protocol-conforming values; the sums mean
// nothing here, memory safety, the sizes of the buffers, the snapshot's life and every error path are the subject.
// Built and run by tests/test_join_support_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_rows.cuh, ig_kernels_join.cuh: device code, not included here)
struct Item {
    long long off;
    int len, pad;
};
struct Long {
    long long off, scratch, len;
};
struct End {
    int start, n;
    float l_kb;
    int pad;
};
enum { NS_ENTRIES = 6, CLS_WORDS = 8 };

static int g_per_contig = 3;    // positions per modelled contig
static long long g_entries = 0; // (contact, link) entries the emit model makes
static u64 g_maxq = 1;          // what the model pass reports as the largest |q|
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
    const int T = *(int*)a[1];
    u64* head = *(u64**)a[2];
    for (int r = 0; r < T; r++) head[r] = r % g_per_contig == 0;
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
static void model_ends(void** a, dim3, dim3)
{
    const int T = *(int*)a[2], K = *(int*)a[3];
    End* ends = *(End**)a[9];
    for (int k = 0; k < K; k++) ends[k] = End{k * g_per_contig, std::min(g_per_contig, T - k * g_per_contig), 1.0f, 0};
}
static void model_records(void** a, dim3, dim3)
{
    const int M = *(int*)a[1];
    int4* rec = *(int4**)a[6];
    for (int s = 0; s < M; s++) rec[s] = make_int4(0, 0, -1, 0);
}
static void model_count(void** a, dim3, dim3)
{
    const int U = *(int*)a[5];
    u64 *counter = *(u64**)a[6], *sc = *(u64**)a[9];
    if (U < 4) return;
    for (long long e = 0; e < g_entries; e++) counter[row_of_entry(e, U)]++;
    sc[NS_ENTRIES] += (u64)g_entries;
    sc[0] += (u64)g_entries;
}
static void model_scatter(void** a, dim3, dim3)
{
    const int U = *(int*)a[5];
    u64 *cursor = *(u64**)a[6], *ent = *(u64**)a[7];
    const u64 n_ent = *(u64*)a[8];
    if (U < 4) return;
    for (long long e = 0; e < g_entries; e++) {
        const u64 lo = row_of_entry(e, U), slot = cursor[lo]++;
        if (slot < n_ent) ent[slot] = ((u64)(lo + 2 + (u64)(e % 3)) << 32) | 1ull;
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
static void model_sort_items(void** a, dim3 grid, dim3) // k_lift_sort_lds: touches every entry of every listed stretch
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
static void model_merge(void** a, dim3 grid, dim3) // k_lift_merge: reads and writes every entry of every long row on both sides
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
static void model_model(void** a, dim3, dim3)
{
    const long long n_links = *(long long*)a[3];
    u64 *pairs = *(u64**)a[10], *expq = *(u64**)a[11], *maxq = *(u64**)a[12];
    for (long long g = 0; g < n_links; g++) pairs[g] = 1, expq[g] = 7;
    *maxq = std::max(*maxq, g_maxq);
}

static int build_and_read(ig_ctx* c, int window, int model, long long want_links)
{
    int64_t n_ends = -7, n_links = -7, sc[8];
    CHECK(ig_join_support_build(c, window, model, &n_ends, &n_links, sc) == 0);
    CHECK(n_ends % 2 == 0 && n_ends >= 0 && n_links == want_links && sc[7] == n_links && sc[6] * 2 == n_ends);
    std::vector<int64_t> rows((size_t)n_ends + 1, -7);
    std::vector<int32_t> first((size_t)n_ends / 2 + 1, -7), npos((size_t)n_ends / 2 + 1, -7);
    CHECK(ig_join_support_rows(c, rows.data(), n_ends) != 0 && std::strstr(ig_last_error(), "capacity") && rows[0] == -7);
    CHECK(ig_join_support_rows(c, rows.data(), n_ends + 1) == 0 && rows[0] == 0 && rows[(size_t)n_ends] == n_links);
    if (n_ends) CHECK(ig_join_support_ends(c, first.data(), npos.data(), n_ends / 2 - 1) != 0 && first[0] == -7);
    CHECK(ig_join_support_ends(c, first.data(), npos.data(), n_ends / 2) == 0);
    std::vector<int32_t> col((size_t)n_links + 1);
    std::vector<int64_t> obs((size_t)n_links + 1), prs((size_t)n_links + 1), exq((size_t)n_links + 1);
    CHECK(ig_join_support_fetch(c, 0, n_links + 1, col.data(), obs.data(), nullptr, nullptr) != 0);
    CHECK(ig_join_support_fetch(c, -1, 1, col.data(), obs.data(), nullptr, nullptr) != 0);
    CHECK(ig_join_support_fetch(c, 0, n_links, col.data(), obs.data(), nullptr, nullptr) == 0);
    if (model) CHECK(ig_join_support_fetch(c, 0, n_links, col.data(), obs.data(), prs.data(), exq.data()) == 0 && (!n_links || (prs[0] == 1 && exq[0] == 7)));
    else CHECK(ig_join_support_fetch(c, 0, n_links, col.data(), obs.data(), prs.data(), exq.data()) != 0 && std::strstr(ig_last_error(), "model = 0"));
    for (int64_t g = 1; g < n_links; g += 97) CHECK(ig_join_support_fetch(c, g, 1, col.data(), obs.data(), model ? prs.data() : nullptr, nullptr) == 0);
    int64_t forms[8];
    CHECK(ig_debug_join_support_forms(c, forms) == 0);
    return 0;
}

int main()
{
    fake_hip::set_model("k_join_heads", model_heads);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_join_ends", model_ends);
    fake_hip::set_model("k_join_records", model_records);
    fake_hip::set_model("k_join_emitILb0E", model_count);
    fake_hip::set_model("k_join_emitILb1E", model_scatter);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_lift_reduce", model_reduce);
    fake_hip::set_model("k_join_model", model_model);

    const Fixture fx;
    const int64_t Z = fx.Z;

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    int64_t n_ends, n_links, sc[8];
    int32_t i32[4];
    int64_t i64[4];
    CHECK(ig_join_support_fetch(c, 0, 0, i32, i64, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    CHECK(ig_join_support_rows(c, i64, 4) != 0 && ig_join_support_ends(c, i32, i32, 4) != 0 && ig_join_support_release(c) == 0);
    const auto fresh_build = [&](bool model) { return n_ends = n_links = -7, ig_join_support_build(c, 64, model, &n_ends, &n_links, sc); };
    if (bring_up_ladder(fx, c, fresh_build, [&] { return n_ends == -7 && n_links == -7; }, true, PARAMS_WITH_MODEL)) return 1;
    CHECK(fx.params(c) == 0);
    for (int bad : {0, 1025, -3}) CHECK(ig_join_support_build(c, bad, 1, &n_ends, &n_links, sc) != 0 && std::strstr(ig_last_error(), "window"));
    CHECK(ig_join_support_build(c, 64, 1, nullptr, &n_links, sc) != 0 && ig_join_support_build(c, 64, 1, &n_ends, &n_links, nullptr) != 0);

    // shapes of the entries: none; a few (rows of the short form); many (lds and long rows under lowered limits)
    for (int per : {3, 1, 80}) {                       // 27, 80 contigs -- and one: K < 2
        g_per_contig = per;
        for (long long entries : {0ll, 50ll, (long long)(4 * Z)}) { // (the host refuses more than four entries per contact)
            g_entries = per == 80 ? 0 : entries;
            for (int limits = 0; limits < 3; limits++) {
                CHECK(ig_debug_assembly_contacts_limits(c, limits == 0 ? 0 : limits == 1 ? 2 : 1, limits == 0 ? 0 : limits == 1 ? 4 : 1) == 0);
                for (int model = 0; model < 2; model++) {
                    CHECK(ig_debug_join_support_combine(c, model) == 0);
                    if (build_and_read(c, 64, model, g_entries)) return 1;
                }
            }
        }
    }
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && ig_debug_join_support_combine(c, -1) == 0);
    g_per_contig = 3;
    g_entries = 4 * Z + 1; // more entries than four per contact: a device error, caught before anything is sized by it
    CHECK(ig_join_support_build(c, 64, 1, &n_ends, &n_links, sc) != 0 && std::strstr(ig_last_error(), "device error"));
    g_entries = 300;
    g_no_heads = true; // no head among the entries: caught too, and no stale result
    CHECK(ig_join_support_build(c, 64, 1, &n_ends, &n_links, sc) != 0 && std::strstr(ig_last_error(), "distinct"));
    CHECK(ig_join_support_fetch(c, 0, 0, i32, i64, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    g_no_heads = false;
    g_free_bytes = 4096; // the entries do not fit what is free: refused with the bytes named, before anything is allocated by their number
    {
        const long before = fake_hip::allocations();
        CHECK(ig_join_support_build(c, 64, 1, &n_ends, &n_links, sc) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
        CHECK(fake_hip::allocations() - before < 16); // (the tables of the ends and the counters only)
        CHECK(ig_join_support_fetch(c, 0, 0, i32, i64, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    }
    g_free_bytes = (size_t)1 << 34;
    g_maxq = 1ull << 50; // times 1024 * 1025 / 2 pairs: beyond 2^62
    CHECK(ig_join_support_build(c, 1024, 1, &n_ends, &n_links, sc) != 0 && std::strstr(ig_last_error(), "model value too large for this window"));
    CHECK(ig_join_support_build(c, 1, 1, &n_ends, &n_links, sc) == 0); // (one pair per link: nothing to overflow)
    CHECK(ig_join_support_build(c, 1024, 0, &n_ends, &n_links, sc) == 0);
    g_maxq = 1;
    // every allocation of a build fails once: an error, nothing leaked, nothing stale, and the next build works
    for (int n = 0; n < 64; n++) {
        fake_hip::fail_allocation_in(n);
        const int rc = ig_join_support_build(c, 64, 1, &n_ends, &n_links, sc);
        fake_hip::fail_allocation_in(-1);
        if (rc) CHECK(ig_join_support_fetch(c, 0, 0, i32, i64, nullptr, nullptr) != 0);
        else CHECK(n_links == 300);
        if (build_and_read(c, 64, 1, 300)) return 1;
    }
    // the time entry point, the lift through the shared functions, a live snapshot through a new upload and through ig_destroy
    std::vector<float> ms(2 * 9);
    int64_t ck = 0;
    CHECK(ig_debug_join_support_time(c, 64, 2, ms.data(), &ck) == 0 && ig_debug_join_support_time(c, 64, 0, ms.data(), &ck) != 0);
    int64_t nu, ne;
    CHECK(ig_assembly_contacts_build(c, 1, &nu, &ne, sc) == 0 || std::strlen(ig_last_error()) > 0);
    CHECK(ig_assembly_contacts_build(c, 0, &nu, &ne, sc) == 0 || std::strlen(ig_last_error()) > 0);
    if (build_and_read(c, 64, 1, 300)) return 1;
    CHECK(fx.contacts(c) == 0);
    CHECK(ig_join_support_fetch(c, 0, 0, i32, i64, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    if (build_and_read(c, 64, 1, 300)) return 1;
    ig_destroy(c);
    std::printf("join harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
