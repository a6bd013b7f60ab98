// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the segment placement support (csrc/ig_host_segplace.inc) with the
// records it shares with the join support (join_enqueue_records), the sort and reduction of the row builder (csrc/ig_host_rows.inc) and the
// placement support's scan: a stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy,
// fill and model write is checked against the real allocation sizes).  The models below script what steers the host -- the number of
// contigs, the verdict on the caller's list, the entries per row, the work lists of the three sort forms, the heads, the sum of the counts
// -- with protocol-conforming values, and touch every word the kernels touch; the sums mean nothing here, memory safety, the sizes of the
// buffers against the work lists, that nothing outlives a call and every error path are the subject.  Built and run by
// tests/test_segment_placement_sanitize.py.
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
enum { NS_COUNTED = 3, NS_ENTRIES = 5, NI = 12, NL = 6, NQ = 12, NSC = 9, PASSES = 11 };

static int g_per_contig = 3;      // positions per modelled contig
static long long g_entries = 0;   // (contact, row) entries the emit model makes
static u64 g_counted = 1000;      // what the count pass reports as the sum of the counted contacts' counts
static bool g_no_heads = false;   // the reduction finds no head: a device error the host must catch
static bool g_many_heads = false; // more contigs than positions: inconsistent tables
static bool g_spans = false;      // the records model finds a segment that spans two contigs
static long g_scans = 0;          // launches of the scan's model
static long g_quadrants = 0;      // launches of the quadrants' model

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
    for (int r = 0; r < T; r++) head[r] = g_many_heads ? 2 : r % g_per_contig == 0;
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
    for (int s = 0; s < M; s++) rec[s] = make_int4(0, 0, s / g_per_contig, s);
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
// k_place_scan: reads the records of every bin, the rows, every summed entry and every prefix sum (one more than the entries), the
// tables by position; writes every word of the output arrays
static void model_scan(void** a, dim3, dim3)
{
    const int4* bins = *(const int4**)a[0];
    const int N = *(int*)a[1];
    const u64* rowptr = *(const u64**)a[2];
    const int* col = *(const int**)a[3];
    const u64* pre = *(const u64**)a[4];
    const long long n_ent = *(long long*)a[5];
    const int2* meta = *(const int2**)a[6];
    const u64* incl = *(const u64**)a[7];
    const int T = *(int*)a[8];
    int* out_i = *(int**)a[13];
    long long* out_l = *(long long**)a[14];
    u64 sum = 0;
    for (int f = 0; f < N; f++) {
        sum += (u64)bins[f].x;
        for (u64 e = rowptr[f]; e < rowptr[f + 1] && e < (u64)n_ent; e++) sum += (u64)col[e] + pre[e + 1] - pre[e];
    }
    sum += pre[n_ent] + rowptr[N];
    for (int r = 0; r < T; r++) sum += (u64)meta[r].y + incl[r];
    for (int k = 0; k < 11; k++) // (the placement support's eleven arrays: the arm is k_segplace_windows')
        for (int f = 0; f < N; f++) out_i[(size_t)k * N + f] = k == 0 ? 0 : (int)(sum & 1) + k;
    for (int k = 0; k < NL; k++)
        for (int f = 0; f < N; f++) out_l[(size_t)k * N + f] = 100 + k;
    g_scans++;
}

// k_segplace_map: the kernel's own search, every position of the genome order written once
static void model_map(void** a, dim3, dim3)
{
    const int *first = *(const int**)a[0], *last = *(const int**)a[1];
    const int n_seg = *(int*)a[2], T = *(int*)a[3];
    int* seg_of = *(int**)a[4];
    for (int r = 0; r < T; r++) {
        int lo = 0, hi = n_seg;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= r) lo = mid + 1;
            else hi = mid;
        }
        seg_of[r] = lo > 0 && last[lo - 1] >= r ? lo - 1 : -1;
    }
}
// k_segplace_records: the list checked as the kernel checks it (range, order; two contigs on the harness's word), a record per segment
static void model_seg_records(void** a, dim3, dim3)
{
    const int *first = *(const int**)a[0], *last = *(const int**)a[1];
    const int n_seg = *(int*)a[2];
    const int2* meta = *(const int2**)a[3];
    const u64* incl = *(const u64**)a[4];
    const int T = *(int*)a[5];
    int4* recs = *(int4**)a[7];
    int* err = *(int**)a[8];
    for (int k = 0; k < n_seg; k++) {
        const int f = first[k], l = last[k];
        int e = 0;
        if (f < 0 || l < f || l >= T) e |= 1;
        if (k > 0 && f <= last[k - 1]) e |= 2;
        if (!e && g_spans) e |= 4;
        recs[k] = e ? make_int4(-1, 0, -2, 0) : make_int4(f, l - f + 1, (int)((incl[f] + (u64)meta[f].x + (u64)meta[l].x) & 0), 0);
        *err |= e;
    }
}
static void model_count(void** a, dim3, dim3)
{
    const int* seg_of = *(const int**)a[4];
    const int T = *(int*)a[5], n_seg = *(int*)a[6];
    u64 *counter = *(u64**)a[7], *sc = *(u64**)a[10];
    u64 sum = 0;
    for (int r = 0; r < T; r++) sum += (u64)seg_of[r];
    for (long long e = 0; e < g_entries; e++) counter[row_of_entry(e, n_seg)]++;
    sc[NS_ENTRIES] += (u64)g_entries;
    sc[NS_COUNTED] += g_counted + (sum & 0);
}
static void model_scatter(void** a, dim3, dim3)
{
    const int n_seg = *(int*)a[6];
    u64 *cursor = *(u64**)a[7], *ent = *(u64**)a[8];
    const u64 n_ent = *(u64*)a[9];
    for (long long e = 0; e < g_entries; e++) {
        const u64 row = row_of_entry(e, n_seg), slot = cursor[row]++;
        if (slot < n_ent) ent[slot] = ((u64)(e % 5) << 32) | 1ull;
    }
}
// k_segplace_windows: reads every record, the scan's eleven arrays and the table of the contigs; writes every window and every arm
static void model_windows(void** a, dim3, dim3)
{
    const int4* recs = *(const int4**)a[0];
    const int n_seg = *(int*)a[1];
    const int* out_i = *(const int**)a[2];
    const End* ends = *(const End**)a[3];
    const int K = *(int*)a[4];
    int4* win = *(int4**)a[7];
    int* arm = *(int**)a[8];
    long long sum = 0;
    for (int k = 0; k < K; k++) sum += ends[k].start + ends[k].n;
    for (int i = 0; i < 11 * n_seg; i++) sum += out_i[i];
    for (int s = 0; s < n_seg; s++) {
        for (int site = 0; site < 3; site++) win[3 * s + site] = make_int4(recs[s].x, recs[s].x + 1, recs[s].x + 2, (int)(sum & 0));
        arm[s] = recs[s].y / 2;
    }
}
// k_segplace_quadrants: reads the segment of every position, every record and every window; adds into every word of the quadrants
static void model_quadrants(void** a, dim3, dim3)
{
    const int* seg_of = *(const int**)a[4];
    const int T = *(int*)a[5], n_seg = *(int*)a[6];
    const int4 *recs = *(const int4**)a[8], *win = *(const int4**)a[9];
    u64* quad = *(u64**)a[10];
    u64 sum = 0;
    for (int r = 0; r < T; r++) sum += (u64)seg_of[r];
    for (int s = 0; s < n_seg; s++) {
        sum += (u64)recs[s].y;
        for (int w = 0; w < 12; w++) quad[12 * (size_t)s + w] += 200 + (u64)win[3 * s + w / 4].x * 0 + (sum & 0);
    }
    g_quadrants++;
}

struct Out {
    std::vector<int32_t> vi;
    std::vector<int64_t> vl, vq;
    int64_t sc[NSC];
    int n;
    explicit Out(int n_seg) : vi((size_t)NI * n_seg + 1, -7), vl((size_t)NL * n_seg + 1, -7), vq((size_t)NQ * n_seg + 1, -7), n(n_seg)
    {
        for (int k = 0; k < NSC; k++) sc[k] = -7;
    }
    int32_t* i(int k) { return vi.data() + (size_t)k * n; }
    int64_t* l(int k) { return vl.data() + (size_t)k * n; }
    bool untouched() const
    {
        const auto is = [](int64_t v) { return v == -7; };
        return std::all_of(vi.begin(), vi.end(), is) && std::all_of(vl.begin(), vl.end(), is) && std::all_of(vq.begin(), vq.end(), is) && sc[0] == -7 && sc[8] == -7;
    }
};

struct List {
    std::vector<int32_t> first, last;
    explicit List(int n_seg, int len = 2)
    {
        for (int k = 0; k < n_seg; k++) first.push_back(k * len), last.push_back(k * len + len - 1);
    }
    int n() const { return (int)first.size(); }
};

static int call(ig_ctx* c, int window, int min_hosts, const List& s, Out& o)
{
    return ig_segment_placement(c, window, min_hosts, s.n(), s.first.data(), s.last.data(), o.vi.data(), o.vl.data(), o.vq.data(), o.sc);
}

static int call_and_read(ig_ctx* c, int window, int min_hosts, const List& s, long long want_entries)
{
    Out o(s.n());
    CHECK(call(c, window, min_hosts, s, o) == 0);
    CHECK(o.sc[NS_ENTRIES] == want_entries && o.sc[7] == s.n() && o.sc[6] >= 0 && o.sc[8] == Fixture::M);
    for (int k = 0; k < s.n(); k++) CHECK(o.i(0)[k] == 0 && o.l(5)[k] == 105 && o.i(10)[k] >= 10 && o.i(11)[k] == (s.last[k] - s.first[k] + 1) / 2 && o.vq[(size_t)NQ * k + 11] == 200);
    CHECK(o.vi.back() == -7 && o.vl.back() == -7 && o.vq.back() == -7); // nothing behind the arrays
    return 0;
}

int main()
{
    fake_hip::set_model("k_join_heads", model_heads);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_join_ends", model_ends);
    fake_hip::set_model("k_join_records", model_records);
    fake_hip::set_model("k_segplace_map", model_map);
    fake_hip::set_model("k_segplace_records", model_seg_records);
    fake_hip::set_model("k_segplace_emitILb0E", model_count);
    fake_hip::set_model("k_segplace_emitILb1E", model_scatter);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_lift_reduce", model_reduce);
    fake_hip::set_model("k_place_scan", model_scan);
    fake_hip::set_model("k_segplace_windows", model_windows);
    fake_hip::set_model("k_segplace_quadrants", model_quadrants);

    const Fixture fx;
    const int64_t Z = fx.Z;
    const List pairs(Fixture::N), none(0), one(1, Fixture::M), few(13, 6);

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    {
        Out o(pairs.n());
        if (bring_up_ladder(fx, c, [&](bool) { return call(c, 64, 64, pairs, o); }, [&] { return o.untouched(); }, true, PARAMS_NEVER)) return 1;
        for (int bad : {0, 1025, -3}) CHECK(call(c, bad, 1, pairs, o) != 0 && std::strstr(ig_last_error(), "window") && o.untouched());
        for (int bad : {0, 129, -1}) CHECK(call(c, 64, bad, pairs, o) != 0 && std::strstr(ig_last_error(), "min_hosts") && o.untouched());
        CHECK(call(c, 1024, 2049, pairs, o) != 0 && call(c, 1, 3, pairs, o) != 0 && o.untouched());
        // NULL arrays, NULL lists, a negative length
        CHECK(ig_segment_placement(c, 64, 64, pairs.n(), pairs.first.data(), pairs.last.data(), nullptr, o.vl.data(), o.vq.data(), o.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_segment_placement(c, 64, 64, pairs.n(), pairs.first.data(), pairs.last.data(), o.vi.data(), nullptr, o.vq.data(), o.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_segment_placement(c, 64, 64, pairs.n(), pairs.first.data(), pairs.last.data(), o.vi.data(), o.vl.data(), nullptr, o.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_segment_placement(c, 64, 64, pairs.n(), pairs.first.data(), pairs.last.data(), o.vi.data(), o.vl.data(), o.vq.data(), nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_segment_placement(c, 64, 64, pairs.n(), nullptr, pairs.last.data(), o.vi.data(), o.vl.data(), o.vq.data(), o.sc) != 0 && std::strstr(ig_last_error(), "NULL segment list"));
        CHECK(ig_segment_placement(c, 64, 64, pairs.n(), pairs.first.data(), nullptr, o.vi.data(), o.vl.data(), o.vq.data(), o.sc) != 0 && std::strstr(ig_last_error(), "NULL segment list"));
        CHECK(ig_segment_placement(c, 64, 64, -1, pairs.first.data(), pairs.last.data(), o.vi.data(), o.vl.data(), o.vq.data(), o.sc) != 0 && std::strstr(ig_last_error(), "-1 entries"));
        CHECK(o.untouched());
        CHECK(ig_set_shard(c, 1, 2) == 0); // a sharded handle: refused before anything is allocated
        const long before = fake_hip::allocations();
        CHECK(call(c, 64, 64, pairs, o) != 0 && std::strstr(ig_last_error(), "all contacts on one handle") && fake_hip::allocations() == before && o.untouched());
        CHECK(ig_set_shard(c, 0, 1) == 0);
        // the segment-list refusals, in the rule's words
        List bad = pairs;
        bad.last[5] = Fixture::M;
        CHECK(call(c, 64, 64, bad, o) != 0 && std::strstr(ig_last_error(), "segment list out of range: 0 <= first <= last < 80") && o.untouched());
        bad = pairs, bad.first[0] = -1;
        CHECK(call(c, 64, 64, bad, o) != 0 && std::strstr(ig_last_error(), "out of range") && o.untouched());
        bad = pairs, bad.last[7] = bad.first[7] - 1;
        CHECK(call(c, 64, 64, bad, o) != 0 && std::strstr(ig_last_error(), "out of range") && o.untouched());
        bad = pairs, bad.first[9] = bad.last[8];
        CHECK(call(c, 64, 64, bad, o) != 0 && std::strstr(ig_last_error(), "segment list not ascending and disjoint") && o.untouched());
        bad = pairs, std::swap(bad.first[3], bad.first[4]), std::swap(bad.last[3], bad.last[4]);
        CHECK(call(c, 64, 64, bad, o) != 0 && std::strstr(ig_last_error(), "not ascending and disjoint") && o.untouched());
        g_spans = true;
        CHECK(call(c, 64, 64, pairs, o) != 0 && std::strstr(ig_last_error(), "segment list: a segment spans two contigs") && o.untouched());
        g_spans = false;
        const List longer(Fixture::M + 1, 1); // more segments than positions: refused before the list is read
        Out q(longer.n());
        CHECK(call(c, 64, 64, longer, q) != 0 && std::strstr(ig_last_error(), "out of range") && q.untouched());
    }

    // shapes of the entries: none; a few (rows of the short form); many (lds and long rows under lowered limits); every form of the scan;
    // lists of many, of a few and of one segment
    for (int per : {3, 1, 80}) { // 27, 80 contigs -- and one
        g_per_contig = per;
        for (const List* s : {&pairs, &few, &one}) {
            for (long long entries : {0ll, 50ll, (long long)(2 * Z)}) { // (the host refuses more than two entries per contact)
                g_entries = entries;
                for (int limits = 0; limits < 3; limits++) {
                    CHECK(ig_debug_assembly_contacts_limits(c, limits == 0 ? 0 : limits == 1 ? 2 : 1, limits == 0 ? 0 : limits == 1 ? 4 : 1) == 0);
                    for (int form = 0; form < 3; form++) {
                        CHECK(ig_debug_placement_support_form(c, form) == 0); // (the scan is the placement support's: so is its setting)
                        const long scans = g_scans, quads = g_quadrants;
                        if (call_and_read(c, 64, 1 + form, *s, g_entries)) return 1;
                        CHECK(g_scans - scans == (form == 0 ? 2 : 1) && g_quadrants - quads == 1);
                    }
                }
            }
        }
    }
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && ig_debug_placement_support_form(c, 0) == 0);
    g_per_contig = 3;
    // n_seg == 0: success with the class sums, nothing read from or written to the arrays (they may be NULL)
    g_entries = 0;
    {
        int64_t sc[NSC];
        const long scans = g_scans, quads = g_quadrants;
        CHECK(ig_segment_placement(c, 64, 64, 0, nullptr, nullptr, nullptr, nullptr, nullptr, sc) == 0 && sc[NS_COUNTED] == 1000 && sc[7] == 0 && sc[8] == Fixture::M);
        CHECK(g_scans == scans && g_quadrants == quads);
        Out o(0);
        CHECK(call(c, 64, 64, none, o) == 0 && o.vi[0] == -7 && o.vl[0] == -7 && o.vq[0] == -7 && o.sc[NS_ENTRIES] == 0);
        g_entries = 2; // entries without a segment to take them
        CHECK(call(c, 64, 64, none, o) != 0 && std::strstr(ig_last_error(), "device error"));
    }
    Out o(pairs.n());
    // the plausibility checks, before anything is sized by what the device reported
    g_entries = 2 * Z + 2; // more entries than two per contact
    CHECK(call(c, 64, 64, pairs, o) != 0 && std::strstr(ig_last_error(), "device error") && o.untouched());
    g_entries = 300;
    g_many_heads = true; // more contigs than positions
    CHECK(call(c, 64, 64, pairs, o) != 0 && std::strstr(ig_last_error(), "inconsistent tables") && o.untouched());
    g_many_heads = false;
    g_no_heads = true; // no head among the entries: caught too
    CHECK(call(c, 64, 64, pairs, o) != 0 && std::strstr(ig_last_error(), "distinct") && o.untouched());
    g_no_heads = false;
    g_free_bytes = 4096; // the entries do not fit what is free: refused with the bytes named, before anything is allocated by their number
    {
        const long before = fake_hip::allocations();
        CHECK(call(c, 64, 64, pairs, o) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && o.untouched());
        CHECK(fake_hip::allocations() - before < 24); // (the records, the list and the counters only)
    }
    g_free_bytes = (size_t)1 << 34;
    // the overflow guard on both sides of 2^62: 2 w sum(counts) >= 2^62
    g_counted = 1ull << 51;
    CHECK(call(c, 1024, 1024, pairs, o) != 0 && std::strstr(ig_last_error(), "counts too large for this window") && o.untouched());
    g_counted = (1ull << 51) - 1000; // (the other classes are 0 here: just below)
    if (call_and_read(c, 1024, 1024, pairs, 300)) return 1;
    g_counted = 1ull << 60;
    CHECK(call(c, 2, 1, pairs, o) != 0 && std::strstr(ig_last_error(), "counts too large for this window"));
    if (call_and_read(c, 1, 1, pairs, 300)) return 1;
    g_counted = 1ull << 62;
    CHECK(call(c, 1, 1, pairs, o) != 0 && std::strstr(ig_last_error(), "counts too large for this window") && o.untouched());
    g_counted = 1000;
    // every allocation of a call fails once: an error, nothing written, nothing leaked, and the next call works
    {
        Out q(pairs.n());
        const auto fresh_outputs = [&] { return q = Out(pairs.n()), call(c, 64, 64, pairs, q); };
        if (allocation_failure_sweep(fx, c, 64, 64, 0, 25, fresh_outputs, [&] { return q.untouched(); }, [&] { return call_and_read(c, 64, 64, pairs, 300) == 0; })) return 1;
    }
    // the time entry point; the placement support, the join support and the lift through the functions they share with this feature
    std::vector<float> ms(2 * PASSES);
    int64_t ck = 0;
    CHECK(ig_debug_segment_placement_time(c, 64, 64, pairs.n(), pairs.first.data(), pairs.last.data(), 2, ms.data(), &ck) == 0 && ck != 0);
    CHECK(ig_debug_segment_placement_time(c, 64, 64, pairs.n(), pairs.first.data(), pairs.last.data(), 0, ms.data(), &ck) != 0);
    CHECK(ig_debug_segment_placement_time(c, 64, 129, pairs.n(), pairs.first.data(), pairs.last.data(), 1, ms.data(), &ck) != 0);
    g_entries = 0; // (an empty list takes no entry)
    CHECK(ig_debug_segment_placement_time(c, 64, 64, 0, nullptr, nullptr, 1, ms.data(), &ck) == 0);
    g_entries = 300;
    CHECK(ig_debug_segment_placement_time(c, 64, 64, -2, nullptr, nullptr, 1, ms.data(), &ck) != 0);
    int64_t nu, ne, sc8[8];
    CHECK(ig_assembly_contacts_build(c, 1, &nu, &ne, sc8) == 0 || std::strlen(ig_last_error()) > 0);
    CHECK(ig_join_support_build(c, 64, 0, &nu, &ne, sc8) == 0 || std::strlen(ig_last_error()) > 0);
    if (call_and_read(c, 64, 64, pairs, 300)) return 1;
    // ig_destroy behind a failed call
    CHECK(failed_call_before_destroy(c, 12, [&] { return call(c, 64, 64, pairs, o); }) != 0);
    std::printf("segplace harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
